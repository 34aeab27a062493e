// abi_sweep.cpp -- one evaluation on the device: launch geometry, the sweep launches of every pool family, the row
// fold.  (How its result crosses to the host, and the pre-armed evaluations: abi_handover.cpp.)
#include "ctx.h"
#include "granule.h"

#include <algorithm>
#include <cstring>

using namespace cfmm;

namespace {

// Large-market mode: token -> (pool, side) incidence in CSR form, cut into chunks of at most
// kGatherChunk entries (hub tokens are spread over many wavefronts), plus the flow scratch.
int build_incidence(cfmm_ctx* c)
{
    const int64_t m = c->m_total;
    if (2 * m > (int64_t)INT32_MAX) return fail(c, CFMM_ERR_UNSUPPORTED, "large-market mode supports up to 2^30 pools");
    std::vector<int> off((size_t)c->n + 1, 0);
    for (const auto& s : c->segs)
        for (int64_t k = 0; k < 2 * s.m; ++k) ++off[(size_t)s.h_ai[(size_t)k] + 1];
    for (int t = 0; t < c->n; ++t) off[(size_t)t + 1] += off[(size_t)t];
    std::vector<int> entries((size_t)(2 * m)), cursor(off.begin(), off.end() - 1);
    for (const auto& s : c->segs)
        for (int64_t i = 0; i < s.m; ++i)
            for (int side = 0; side < 2; ++side)
                entries[(size_t)cursor[(size_t)s.h_ai[(size_t)(2 * i + side)]]++] = (int)(2 * (s.trade_off + i) + side);
    std::vector<int2> chunks;
    std::vector<int> tok_chunk_off((size_t)c->n + 1, 0);
    for (int t = 0; t < c->n; ++t) {
        for (int b = off[(size_t)t]; b < off[(size_t)t + 1]; b += kGatherChunk)
            chunks.push_back(make_int2(b, std::min(b + kGatherChunk, off[(size_t)t + 1])));
        tok_chunk_off[(size_t)t + 1] = (int)chunks.size();
    }
    // all five go before the first of the new ones comes (the old and the new incidence never coexist)
    c->d_flow.reset(); c->d_entries.reset(); c->d_chunks.reset(); c->d_tok_chunk_off.reset(); c->d_chunk_sums.reset();
    c->n_chunks = (int)chunks.size();
    int rc;
    if ((rc = c->d_entries.upload(c, entries.data(), entries.size())) ||
        (rc = c->d_chunks.upload(c, chunks.data(), chunks.size())) ||
        (rc = c->d_tok_chunk_off.upload(c, tok_chunk_off.data(), tok_chunk_off.size())) ||
        (rc = c->d_flow.alloc(c, (size_t)m)) || (rc = c->d_chunk_sums.alloc(c, chunks.size())))
        return rc;
    return CFMM_OK;
}

} // namespace

namespace cfmm {

void KernelTimer::take_events(hipEvent_t& a, hipEvent_t& b)
{
    hipEvent_t* out[2] = {&a, &b};
    for (hipEvent_t* e : out) {
        if (used == pool.size()) {
            Event fresh;
            if (fresh.create() == hipSuccess) pool.push_back(std::move(fresh));
        }
        *e = used < pool.size() ? pool[used++].get() : nullptr;
    }
    if (!a || !b) a = b = nullptr;
}

// The launch plan of the current segments (launch_plan.h), then what needs the device: the launches' fee tables and the buffers.
int ensure_geometry(cfmm_ctx* c)
{
    if (!c->geometry_dirty) return CFMM_OK;
    std::vector<PlanSeg> shapes;
    for (const Segment& s : c->segs)
        shapes.push_back({s.kind, s.m, s.n_coins, s.n_ticks_total, s.u.has_walk, (bool)s.pk, (int)s.gvals.size()});
    LaunchPlan plan = plan_launches(shapes, c->n, c->geo);
    for (size_t i = 0; i < c->segs.size(); ++i) static_cast<SegPlan&>(c->segs[i]) = plan.segs[i];
    c->groups = std::move(plan.groups);
    c->any_ragged = plan.any_ragged;
    c->rows_total = plan.rows;
    c->m_total = plan.pools;
    c->trade_rows = plan.trades;
    c->flat_total = plan.flat;
    c->touched_bytes = plan.touched_bytes;
    // fee tables of the launches, one kMaxFeeTable slot each
    std::vector<double> tabs(c->groups.size() * (size_t)kMaxFeeTable, 1.0);
    for (size_t gi = 0; gi < c->groups.size(); ++gi) {
        const Group& g = c->groups[gi];
        for (int k = 0; k < g.nseg && g.gtab_n != 0; ++k) {
            const Segment& sg = c->segs[(size_t)g.first + k];
            std::copy(sg.gvals.begin(), sg.gvals.end(), tabs.begin() + (std::ptrdiff_t)(gi * kMaxFeeTable + (size_t)sg.gbase));
        }
    }
    // ... followed, in the same array, by the launches' descriptors (sweep.h SweepDesc; ensure_desc fills them in)
    size_t desc_bytes = 0;
    for (const Group& g : c->groups)
        if (!ragged_kind(c->segs[(size_t)g.first].kind)) desc_bytes += sweep_desc_bytes(g.grid);
    c->desc.base = tabs.size() * sizeof(double);   // (a multiple of 128: kMaxFeeTable doubles per launch)
    c->desc.bytes = desc_bytes;
    int rc = c->d_gtab.grow(c, tabs.size() + desc_bytes / sizeof(double));
    if (rc != CFMM_OK) return rc;
    if (!tabs.empty()) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(c->d_gtab.get(), tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const size_t partials = (size_t)plan.rows * (size_t)row_width(c);
    if (partials > c->d_partials.size()) {
        if ((rc = c->d_partials.grow(c, partials)) != CFMM_OK) return rc;
        HIP_TRY(c, hipMemset(c->d_partials.get(), 0, partials * sizeof(double)));
    }
    const size_t trades = (size_t)plan.trades;   // (two-coin rows only)
    if ((rc = c->d_delta.grow(c, trades)) || (rc = c->d_lambda.grow(c, trades)) || (rc = c->d_over.grow(c, trades))) return rc;
    if (global_bins(c) && (rc = build_incidence(c)) != CFMM_OK) return rc;
    c->geometry_dirty = false;
    c->desc_dirty = true;
    c->have_trades = false;
    c->x_valid = false;
    c->have_out = false;
    return CFMM_OK;
}
namespace {

// What the launches of one evaluation share (enqueue_sweep)
struct Eval {
    const double* d_v;
    double* d_out;
    bool materialize;
    int price_window;
    // large-market mode; fold + all-reduce over the peer mappings in one launch; the sweep's only block publishes {Ψ, acc}
    // itself (no fold); harvest with cfmm_kernel_times
    bool gb, sharded, direct, timed;
    ArmWord arm;
    HostOut ho;
};

// the option "geomean_exact" form of a kind: neither log v from LDS nor a fast arithmetic
bool exact_form(const cfmm_ctx* c, int kind) { return kind_info(kind).exact_form && c->geo.geomean_exact != 0; }

// a launch of one block needs no fold: its row goes straight to the consumer (single-GPU contexts: a sharded fold also
// exchanges, and RCCL all-reduces d_out behind the fold)
bool direct_launch(const cfmm_ctx* c)
{
    return c->groups.size() == 1 && c->groups[0].grid == 1 && !c->groups[0].multi && !global_bins(c) && c->peers.empty() &&
           !ragged_kind(c->segs[(size_t)c->groups[0].first].kind);
}

// What every launch of group g (the gi-th) reads and no evaluation changes: the head of its descriptor (sweep.h SweepDesc)
SweepDesc desc_head(const cfmm_ctx* c, const Group& g, size_t gi)
{
    const bool gb = global_bins(c);
    SweepDesc d;
    std::memset(&d, 0, sizeof d);
    d.n = c->n;
    d.n_pad = c->n_pad;
    d.v_shift = stage_pairs(c->n, g.block) ? 4 : 3;
    d.gtab = c->d_gtab ? c->d_gtab.get() + gi * kMaxFeeTable : nullptr;
    d.gtab_n = d.gtab ? g.gtab_n : 0;
    for (int k = 0; k < g.nseg && !gb; ++k) {
        const int kind = c->segs[(size_t)g.first + k].kind;
        if (kind_info(kind).logv && !exact_form(c, kind)) d.need_logv = 1;
    }
    if (d.need_logv && sweep_lds_bytes(c->n_pad, 1, g.block, 1, d.gtab_n, d.v_shift == 4 ? 1 : 0) > 160 * 1024)
        d.need_logv = 0;   // the log-price row does not fit next to v and one bin copy: one logarithm per pool instead
    d.copies = bin_copies(c->n, c->geo, g.block);
    d.compact = (c->opt_compact_trades != 0 && !gb) ? 1 : 0;
    d.partials = c->d_partials.get() + (size_t)g.row_off * row_width(c);
    d.row_pitch = row_width(c);
    d.flags = c->stage.buf.dev() ? reinterpret_cast<unsigned long long*>(c->stage.buf.dev() + c->stage.flag_off) : nullptr;
    d.nt_stores = c->opt_stream_stores == 2 || (c->opt_stream_stores == 0 && c->touched_bytes > (int64_t)256 << 20) ? 1 : 0;
    d.direct = direct_launch(c) ? 1 : 0;
    return d;
}

// a two-coin segment's pool streams (its member of AnyPools)
AnyPools pools_of(const cfmm_ctx* c, const Segment& s, int gtab_n)
{
    const int gbase = gtab_n ? s.gbase : -1;   // -1: fees from the gamma array
    AnyPools p;
    std::memset(&p, 0, sizeof p);
    switch (s.kind) {
    case CFMM_KIND_PRODUCT:
    case CFMM_KIND_SOLIDLY: p.p = ProductPools{s.R.get(), s.gamma.get(), s.Ai.get(), s.pk.get(), gbase}; break;
    case CFMM_KIND_GEOMEAN:
        p.g = GeoMeanPools{s.R.get(), s.w.get(), s.gamma.get(), s.Ai.get(), s.eta.get(), s.lR.get(), (int)c->geo.geomean_exact,
                           s.pk.get(), gbase};
        break;
    default: {
        const UniV3State& u = s.u;
        p.u = UniV3Pools{u.pg.get(), s.Ai.get(), u.cur_a.get(), u.cur_b.get(), u.cur_c.get(), u.curR.get(), u.walk.get(),
                         u.ticks.get(), u.thr.get(), c->opt_univ3_heads != 0 ? u.head.get() : nullptr, u.has_walk, u.cp.get(),
                         s.pk.get(), gbase};
        break;
    }
    }
    return p;
}

// The descriptors of the current geometry on the device, behind the fee tables in d_gtab (ctx.h SweepDescStore): rebuilt when something they copy has
// changed -- desc_dirty (the geometry, an option, the peers, the stream, a swapped pool array), or a device array or pinned
// buffer of the library created or released since (resource_epoch: a descriptor must never outlive an address it holds) --
// and uploaded in stream order.  The steady state is the two comparisons of the first line.
int ensure_desc(cfmm_ctx* c)
{
    SweepDescStore& ds = c->desc;
    if (!c->desc_dirty && ds.epoch == resource_epoch()) return CFMM_OK;
    const bool gb = global_bins(c);
    ds.heads.clear();
    std::vector<int> kinds;
    for (const Segment& s : c->segs) kinds.push_back(s.kind);
    for (size_t gi = 0; gi < c->groups.size(); ++gi) {
        const Group& g = c->groups[gi];
        SweepDesc d = desc_head(c, g, gi);
        d.nseg = ragged_kind(c->segs[(size_t)g.first].kind) ? 0 : g.nseg;   // 0: sweep_ncoin takes plain arguments
        for (int k = 0; k < d.nseg; ++k) {
            const Segment& s = c->segs[(size_t)g.first + k];
            SegRec& r = d.seg[k];
            r.pools = pools_of(c, s, d.gtab_n);
            r.m = s.m;
            r.Delta = c->d_delta.get() + s.trade_off;
            r.Lambda = c->d_lambda.get() + s.trade_off;
            r.Over = c->d_over.get() + s.trade_off;
            r.gflow = gb ? c->d_flow.get() + s.trade_off : nullptr;
        }
        ds.heads.push_back(d);
    }
    const std::vector<unsigned char> bytes = build_sweep_desc(c->groups, ds.heads, kinds, ds.off);
    if (bytes.size() != ds.bytes || (ds.base + ds.bytes) > c->d_gtab.size() * sizeof(double))
        return fail(c, CFMM_ERR_STATE, "sweep descriptors: %zu bytes built, room for %zu", bytes.size(), ds.bytes);
    // The staging buffer may still be the source of the previous upload: wait for that copy.  The wait is bounded by the
    // work that was on the stream in front of the copy.  That can include a pre-armed launch, but never one that is still
    // waiting for its prices: cfmm_route has at most one such launch pending and signals or cancels it before it enqueues
    // anything else (armed_eval, armed_cancel), and every other entry point cancels a pending launch first.
    if (ds.in_flight) HIP_TRY(c, hipEventSynchronize(ds.uploaded.get()));
    ds.in_flight = false;
    int rc;
    if ((rc = ds.stage.grow(c, bytes.size(), false)) || (rc = ds.uploaded.create(c, hipEventDisableTiming))) return rc;
    if (!bytes.empty()) {
        std::memcpy(ds.stage.host(), bytes.data(), bytes.size());
        HIP_TRY(c, hipMemcpyAsync(ds.dev(c), ds.stage.host(), bytes.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(ds.uploaded.get(), c->stream));
        ds.in_flight = true;
    }
    ds.epoch = resource_epoch();
    c->desc_dirty = false;
    return CFMM_OK;
}

// The kernel's arithmetic (LaunchCfg::arith).  Fast: every pool constant of the launch inside the window (checked at upload),
// prices staged as {v, rcp(v)} pairs, and the prices themselves inside it as far as the host knows ...
int arith_of(const cfmm_ctx* c, const Eval& ev, const Group& g, const SweepDesc& d)
{
    bool fast = c->opt_fast_math != 0 && !ev.gb && d.v_shift == 4 && ev.price_window != kPricesOutside;
    for (int k = 0; k < g.nseg && fast; ++k) {
        const Segment& s = c->segs[(size_t)g.first + k];
        fast = s.fast_ok != 0 && kind_info(s.kind).has_fast && !exact_form(c, s.kind);
    }
    // ... which the host knows for host-pointer sweeps and cfmm_route (pre-armed launches: armed_eval checks the prices before
    // it signals and cancels a launch whose prices turn out to be outside); a device-pointer sweep (prices unknown) gets the
    // kernel that carries both loops and decides per block from the prices it stages
    return !fast ? 0 : (ev.price_window == kPricesUnknown && ev.arm.seq == 0 && c->opt_dev_prices_in_window == 0) ? 2 : 1;
}

// What differs from one evaluation to the next: the kernels' argument
SweepLaunch launch_args(const cfmm_ctx* c, const Eval& ev, size_t gi)
{
    SweepLaunch la;
    std::memset(&la, 0, sizeof la);
    la.desc = c->desc.off[gi] == kNoDesc ? nullptr : reinterpret_cast<const SweepDesc*>(c->desc.dev(c) + c->desc.off[gi]);
    la.v = ev.d_v;
    la.n = c->n;
    la.reverse = c->opt_alternate != 0 ? (int)(c->sweep_count & 1) : 0;
    la.tail.arm_word = ev.arm.word;
    la.tail.arm_seq = ev.arm.seq;
    la.tail.arm_timeout = std::min<long long>(std::max<long long>(c->opt_arm_timeout_ms, 1), 10000) * 100000ll;   // ms -> ticks of the 100 MHz wall clock, at most 10 s
    // sharded (cfmm_set_peers): a rank whose host is late by less than the peer timeout must not lose the evaluation --
    // the other ranks' fold + gather launches wait that long for its granules anyway, so waiting for the price vector
    // equally long turns a stalled host into a slow evaluation on every rank instead of a failed route on all of them
    if (ev.sharded) la.tail.arm_timeout = std::max<long long>(la.tail.arm_timeout, c->peer_timeout_ticks);
    if (ev.direct) {
        la.tail.direct_out = ev.d_out;
        la.tail.direct_host = ev.ho;
        la.reverse = 0;   // two tiles at most, the whole market in one CU's L1: nothing for the alternation to reuse -- and every
                          // evaluation of such a market, fused or materialising, then returns the same bits at the same prices
    }
    return la;
}

// An N-coin segment's launch keeps plain arguments (sweep_ncoin): the head's fields and the launch's in one SweepArgs
SweepArgs ncoin_args(const SweepDesc& d, const SweepLaunch& la, const Segment& s)
{
    SweepArgs a;
    std::memset(&a, 0, sizeof a);
    a.v = la.v;
    a.n = d.n;
    a.n_pad = d.n_pad;
    a.v_shift = d.v_shift;
    a.need_logv = d.need_logv;
    a.gtab = d.gtab;
    a.gtab_n = d.gtab_n;
    a.copies = d.copies;
    a.flags = d.flags;
    a.m = s.m;
    a.compact = d.compact;
    a.partials = d.partials;
    a.row_pitch = d.row_pitch;
    a.reverse = la.reverse;
    a.arm_word = la.tail.arm_word;
    a.arm_seq = la.tail.arm_seq;
    a.arm_timeout = la.tail.arm_timeout;
    a.nt_stores = d.nt_stores;
    return a;
}

// One sweep launch: launch group g, the gi-th of the evaluation
int launch_group(cfmm_ctx* c, const Eval& ev, const Group& g, size_t gi)
{
    const SweepDesc& d = c->desc.heads[gi];
    const SweepLaunch la = launch_args(c, ev, gi);
    const size_t lds = ev.gb ? (size_t)(g.block / 64) * sizeof(double)
                             : sweep_lds_bytes(c->n_pad, d.copies, g.block, d.need_logv, d.gtab_n, d.v_shift == 4 ? 1 : 0);
    hipEvent_t ea = nullptr, eb = nullptr;
    if (ev.timed) c->timer.take_events(ea, eb);   // start/stop written by the command processor around this launch (hipExtLaunchKernel)
    const int arith = arith_of(c, ev, g, d);
    int kinds[kMaxMulti] = {0};
    for (int k = 0; k < d.nseg; ++k) kinds[k] = c->segs[(size_t)g.first + k].kind;
    const bool lean = c->opt_lean_kernels != 0 && lean_launch(d, g, kinds, arith);
    const LaunchCfg cfg{g.block, g.grid, lds, arith, lean, ea, eb};
    const Segment& s0 = c->segs[(size_t)g.first];
    hipError_t e;
    if (g.multi) {
        e = launch_multi(ev.gb, la, cfg, ev.materialize, c->stream);
    } else if (ragged_kind(s0.kind)) {
        const NCoinPools p{s0.nc.R.get(), s0.nc.q.get(), s0.nc.tok.get(), s0.nc.glg.get(), s0.nc.par.get(), s0.n_coins,
                           ev.materialize ? s0.nc.D.get() : nullptr, ev.materialize ? s0.nc.L.get() : nullptr};
        e = launch_ncoin(s0.kind, p, ncoin_args(d, la, s0), ev.gb, cfg, ev.materialize, c->stream);
    } else {
        e = launch_sweep(s0.kind, c->geo.geomean_exact != 0, c->opt_univ3_heads != 0 && s0.u.head, ev.gb, la, cfg, ev.materialize,
                         c->stream);
    }
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "sweep launch failed: %s", hipGetErrorString(e));
    if (ea && eb) c->timer.pending.push_back({ea, eb, 0});
    if (lean) ++c->lean_launches;
    return CFMM_OK;
}

// The row fold behind the sweeps: {Ψ, acc} to ev.d_out (and, ev.ho set, to the host as granules)
int launch_fold(cfmm_ctx* c, const Eval& ev)
{
    hipEvent_t ra = nullptr, rb = nullptr;
    const bool bracket = ev.gb || (c->rows_total == 0 && !ev.sharded);   // several launches / a memset: bracket them with plain events
    if (ev.timed && !ev.direct) c->timer.take_events(ra, rb);
    if (ra && bracket) HIP_TRY(c, hipEventRecord(ra, c->stream));
    hipEvent_t ka = bracket ? nullptr : ra, kb = bracket ? nullptr : rb;   // else: written by the command processor around the fold
    const int rows = (int)c->rows_total, n1 = c->n + 1;
    if (ev.direct) {
        // (the sweep's only block has published {Ψ, acc} itself)
    } else if (ev.sharded) {
        PeerSet ps;
        std::memset(&ps, 0, sizeof ps);
        for (size_t p = 0; p < c->peers.size(); ++p)
            ps.gran[p] = reinterpret_cast<unsigned long long*>(c->peers[p]);
        ps.world = (int)c->peers.size();
        ps.rank = c->peer_rank;
        ps.count = n1;
        ps.seq = ++c->peer_seq;
        ps.timeout_ticks = c->peer_timeout_ticks;
        ps.host = ev.ho;
        ps.arm = ev.arm;
        // a world of ONE rank has nobody to exchange with: the plain fold (same columns, same order; measured 0.6 us per step
        // less than the gather launch with its 200-byte peer table -- N = 1 under a launcher then costs what plain N = 1 costs)
        hipError_t e = (ps.world == 1 && rows > 0 && !ev.gb)
            ? launch_reduce(c->d_partials.get(), rows, n1, row_width(c), ev.d_out, c->stream, ka, kb, ev.ho, ev.arm)
            : launch_reduce_gather(c->d_partials.get(), rows, n1, row_width(c), ev.d_out, c->stream, ps, ka, kb);
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "fold + gather launch failed: %s", hipGetErrorString(e));
    } else if (rows > 0) {
        hipError_t e;
        if (ev.gb) { // pull Ψ per token over the incidence list, then fold the dual-scalar column
            e = launch_gather(c->d_chunks.get(), c->d_entries.get(), reinterpret_cast<const double*>(c->d_flow.get()),
                              c->d_chunk_sums.get(), c->n_chunks, c->d_tok_chunk_off.get(), ev.d_out, c->n, c->d_partials.get(), rows,
                              c->stream);
        } else {
            e = launch_reduce(c->d_partials.get(), rows, n1, row_width(c), ev.d_out, c->stream, ka, kb, ev.ho, ev.arm);
        }
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "reduce launch failed: %s", hipGetErrorString(e));
    } else {
        HIP_TRY(c, hipMemsetAsync(ev.d_out, 0, (size_t)n1 * sizeof(double), c->stream));
    }
    if (ra && rb) {
        if (bracket) HIP_TRY(c, hipEventRecord(rb, c->stream));
        c->timer.pending.push_back({ra, rb, 1});
    }
    return CFMM_OK;
}

} // namespace

// Enqueue one full evaluation on c->stream: every segment's sweep, then the row fold.
//   want_host_out: the fold delivers {Ψ, acc} to the pinned staging buffer as self-validating granules (the caller
//                  polls them: HostStage::wait) instead of writing d_out;
//   arm_seq != 0:  pre-armed launch (SweepArgs::arm_word): v arrives later through c->arm.buf.
//   price_window:  what the host knows about v -- kPricesInWindow (host-pointer sweeps whose prices lie inside the
//                  window of the fast arithmetic), kPricesOutside, or kPricesUnknown (device-pointer sweeps, pre-armed
//                  launches: the fast kernel is launched and its blocks verify, see sweep_tiles).
int enqueue_sweep(cfmm_ctx* c, const double* d_v, double* d_out, bool materialize, bool want_host_out, uint64_t arm_seq,
                  int price_window)
{
    int rc = ensure_geometry(c);
    if (rc != CFMM_OK) return rc;
    Eval ev{d_v, d_out, materialize, price_window};
    ev.gb = global_bins(c);
    ev.sharded = !c->peers.empty();
    ev.timed = c->opt_time_kernels != 0 && c->timer.pending.size() < (1u << 20);
    ev.arm = ArmWord{arm_seq ? c->arm.word() : nullptr, arm_seq};
    const bool rccl = c->rccl_comm != nullptr;   // the fold's {Ψ, acc} are this rank's part: all-reduced in-stream behind it
    const bool host_out = want_host_out && !ev.gb && !rccl && (ev.sharded || c->rows_total > 0) && c->stage.buf.dev() != nullptr;
    if (host_out) {
        ev.ho.gran = reinterpret_cast<unsigned long long*>(c->stage.buf.dev() + c->stage.gran_off);
        ev.ho.tag = granule_tag(++c->stage.out_seq);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_desc(c)) != CFMM_OK) return rc;
    ev.direct = direct_launch(c);
    for (size_t gi = 0; gi < c->groups.size(); ++gi)
        if ((rc = launch_group(c, ev, c->groups[gi], gi)) != CFMM_OK) return rc;
    c->stage.last_host_out = host_out;
    if ((rc = launch_fold(c, ev)) != CFMM_OK) return rc;
    // the sweep and its fold ARE on the stream from here on: the context's bookkeeping says so whatever the collective does
    if (materialize) {
        c->have_trades = true;
        c->x_valid = false;
        c->trades_compact = (c->opt_compact_trades != 0 && !ev.gb) ? 1 : 0;
    }
    ++c->sweep_count;
    if (rccl) {   // north_star: "RCCL all-reduce of Ψ and ∇g over xGMI per outer iteration" -- n + 1 doubles, on the same stream
        rc = rccl_all_reduce_out(c, d_out);
        if (rc != CFMM_OK) {
            c->have_out = false;   // d_out holds this rank's LOCAL {Ψ, acc}, not the market's: nothing may be read from it
            return rc;
        }
    }
    return CFMM_OK;
}

} // namespace cfmm

extern "C" {

int cfmm_sweep_dev(cfmm_ctx* c, const double* d_v, double* d_out, int materialize)
{
    if (!c || !d_v || !d_out) return CFMM_ERR_INVALID_ARG;
    CFMM_SINGLE_ONLY(c, "cfmm_sweep_dev");
    c->have_out = false; // results live on the device; the host copy is stale
    if (materialize) c->trade_v.clear();   // the library has not seen these prices
    // The library cannot see these prices: the launch carries both arithmetics and every block picks from the prices it
    // stages (sweep_core.h kArithAuto) -- prices outside [2^-150, 2^150], NaN included, take the full-range loop and
    // propagate like the reference's arithmetic.  (Round 4 launched the fast kernels on trust and reported a refusal on a
    // LATER call: ADVICE r4.)
    return enqueue_sweep(c, d_v, d_out, materialize != 0, false, 0, kPricesUnknown);
}

} // extern "C"
