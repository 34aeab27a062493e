// abi_update.cpp -- sparse pool-state updates (include/cfmm_amd.h: cfmm_pools_set_reserves, cfmm_pools_set_curve,
// cfmm_pools_set_prices, cfmm_pools_set_ticks): the reference's `cfmm.R .= ...` on a few pools of a router -- and a UniV3
// mint / burn, a pool's new tick ladder -- without re-uploading the market.
// Every row is checked with the upload's own checks (pool_checks.h) before anything changes; the prepared constants are
// computed on the host with the upload's own expressions (pool_checks.h, univ3_pool.h), packed column by column into the
// context's pinned staging buffer and scattered into the segment's columns by ONE launch (sweep.h ScatterArgs) on the
// context's stream.  A moved UniV3 pool's walk lists are appended at the tail of the segment's record arrays; when the tail
// is full the records are compacted on the device (compact_walks).
#include "ctx.h"
#include "pool_checks.h"

#include <algorithm>
#include <cstring>

using namespace cfmm;

namespace {

enum Entry { kSetReserves, kSetCurve, kSetPrices, kSetTicks };
const char* const kEntryName[] = {"cfmm_pools_set_reserves", "cfmm_pools_set_curve", "cfmm_pools_set_prices", "cfmm_pools_set_ticks"};

struct Update {
    Entry entry;
    int32_t seg;
    int64_t count;
    const int64_t* idx;
    const double* R;        // [count][n_coins]        (kSetReserves, kSetCurve)
    const double* alpha;    // [count]                 (kSetCurve)
    const double* beta;
    const double* price;    // [count]                 (kSetPrices, kSetTicks)
    const int64_t* tick_off; // [count + 1]            (kSetTicks: the rows' new ladders in CSR form, as cfmm_pools_add_univ3)
    const double* lt;       // [tick_off[count]]
    const double* liq;
};
const double kNoTick = 0.0;
bool univ3_entry(Entry e) { return e == kSetPrices || e == kSetTicks; }

Entry entry_of_kind(int kind) { return kind == CFMM_KIND_UNIV3 ? kSetPrices : kind == CFMM_KIND_CURVE ? kSetCurve : kSetReserves; }

// the entry fits the segment's kind, or the refusal that names the one that does
int check_entry(const cfmm_ctx* c, Entry entry, int kind)
{
    const Entry right = entry_of_kind(kind);
    if (entry == right || (entry == kSetTicks && kind == CFMM_KIND_UNIV3)) return CFMM_OK;
    return fail(c, CFMM_ERR_INVALID_ARG, "%s: segment of %s pools: %s", kEntryName[entry], kind_info(kind).name, kEntryName[right]);
}

int check_args(const cfmm_ctx* c, const Update& u, int64_t n_segs)
{
    if (u.count < 0) return fail(c, CFMM_ERR_INVALID_ARG, "negative pool count");
    if (u.seg < 0 || u.seg >= n_segs) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    return CFMM_OK;
}
int check_arrays(const cfmm_ctx* c, const Update& u)
{
    const bool ok = u.idx && (univ3_entry(u.entry) ? u.price != nullptr : u.R != nullptr) && (u.entry != kSetCurve || (u.alpha && u.beta)) &&
                    (u.entry != kSetTicks || (u.tick_off && u.lt && u.liq));
    if (u.count > 0 && !ok) return fail(c, CFMM_ERR_INVALID_ARG, "null pool array");
    if (u.count > 0 && u.entry == kSetTicks && u.tick_off[0] != 0) return fail(c, CFMM_ERR_INVALID_ARG, "tick_off[0] must be 0");
    return CFMM_OK;
}

struct Rows {
    std::vector<int64_t> idx, src;
};
Rows distinct_rows(int64_t count, const int64_t* idx);

// Every check of one single-device update, nothing changed: the rows in the caller's order, each with the checks of the
// matching cfmm_pools_add_* on the values given.  row_base: what a shard adds to its rows in error texts (the parent's rows).
int validate(const cfmm_ctx* c, const Update& u, int64_t row_base)
{
    int rc = check_args(c, u, (int64_t)c->segs.size());
    if (rc != CFMM_OK) return rc;
    const Segment& s = c->segs[(size_t)u.seg];
    if ((rc = check_entry(c, u.entry, s.kind)) != CFMM_OK || (rc = check_arrays(c, u)) != CFMM_OK) return rc;
    const int nc = ragged_kind(s.kind) ? s.n_coins : 2;
    for (int64_t j = 0; j < u.count; ++j) {
        const int64_t i = u.idx[j], row = row_base + i;
        if (i < 0 || i >= s.m) return fail(c, CFMM_ERR_INVALID_ARG, "pool index %lld out of range [0, %lld)", (long long)row, (long long)(row_base + s.m));
        if (u.entry == kSetPrices) {
            int64_t ct;
            if ((rc = check_univ3_price(c, row, u.price[j])) != CFMM_OK ||
                (rc = check_univ3_tick(c, row, s.lad.lower_ticks(i), s.lad.count(i), u.price[j], ct)) != CFMM_OK)
                return rc;
            continue;
        }
        if (u.entry == kSetTicks) {   // univ3_build's checks of a pool's state, in its order
            int64_t ct;
            const int64_t o = u.tick_off[j], nt = u.tick_off[j + 1] - o;
            if (nt < 1) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: needs at least one tick", (long long)row);
            if ((rc = check_univ3_price(c, row, u.price[j])) != CFMM_OK ||
                (rc = check_univ3_ladder(c, row, u.lt + o, u.liq + o, nt)) != CFMM_OK ||
                (rc = check_univ3_tick(c, row, u.lt + o, nt, u.price[j], ct)) != CFMM_OK)
                return rc;
            continue;
        }
        const double* R = u.R + j * nc;
        if ((rc = check_reserves(c, row, R, nc)) != CFMM_OK) return rc;
        if (s.kind == CFMM_KIND_SOLIDLY && (rc = check_solidly_range(c, row, R)) != CFMM_OK) return rc;
        if (s.kind == CFMM_KIND_CURVE && (rc = check_curve_params(c, row, u.alpha[j], u.beta[j], R, nc)) != CFMM_OK) return rc;
    }
    if (u.entry == kSetTicks && u.count > 0) {   // the segment's limit (univ3_build) on the new total: every row's last occurrence counts
        const Rows rows = distinct_rows(u.count, u.idx);
        int64_t T = s.lad.ticks_total();
        for (size_t k = 0; k < rows.idx.size(); ++k)
            T += (u.tick_off[rows.src[k] + 1] - u.tick_off[rows.src[k]]) - s.lad.count(rows.idx[k]);
        if (2 * (T + 2 * s.m) > (int64_t)0x3fffffff) return fail(c, CFMM_ERR_UNSUPPORTED, "too many ticks in one segment");
    }
    return CFMM_OK;
}

// The distinct rows of an update in ascending order, each with the position of its LAST occurrence in the caller's arrays
// (a row named twice takes its last value; decided here, on the host, so the result does not depend on the launch)
Rows distinct_rows(int64_t count, const int64_t* idx)
{
    std::vector<std::pair<int64_t, int64_t>> a((size_t)count);
    for (int64_t j = 0; j < count; ++j) a[(size_t)j] = {idx[j], j};
    std::sort(a.begin(), a.end());
    Rows r;
    for (size_t k = 0; k < a.size(); ++k)
        if (k + 1 == a.size() || a[k + 1].first != a[k].first) {
            r.idx.push_back(a[k].first);
            r.src.push_back(a[k].second);
        }
    return r;
}

// Columns of one scatter launch, laid out in the staging buffer in the order they are added
struct Packer {
    ScatterArgs a{};
    unsigned long long* h;
    explicit Packer(cfmm_ctx* c) : h(c->upd.buf.host()) { a.stage = c->upd.buf.dev(); }
    // -> the host side of a column of `rows` rows, `width` words each
    template <class T>
    T* add(void* dst, int width, int64_t rows, int64_t dense_base = -1)
    {
        ScatterCol& col = a.col[a.ncols++];
        a.total = (a.total + 7) & ~7ll;   // every column on a 64-byte boundary of the staging buffer
        col.dst = static_cast<unsigned long long*>(dst);
        col.begin = a.total;
        col.rows = rows;
        col.dense_base = dense_base;
        col.width = width;
        T* p = reinterpret_cast<T*>(h + a.total);
        a.total += rows * width;
        return p;
    }
    // the rows themselves, after the columns
    void set_rows(const std::vector<int64_t>& idx)
    {
        std::memcpy(h + a.total, idx.data(), idx.size() * 8);
        a.idx = reinterpret_cast<const long long*>(a.stage + a.total);
    }
};

int launch(cfmm_ctx* c, const Packer& p)
{
    HIP_TRY(c, launch_scatter_records(p.a, c->stream));
    HIP_TRY(c, hipEventRecord(c->upd.done.get(), c->stream));
    c->upd.busy = true;
    return CFMM_OK;
}

// Room for `need` more records at the tail of a UniV3 segment's ticks / thr.  When it runs out the records in use are compacted
// ON THE DEVICE: the host lays the pools' spans out tightly in pool order (O(m), from its copy of `walk`; the lists of moved
// pools are garbage), stages the new spans in the pinned buffer, and one compact_walks launch copies every pool's records
// into fresh arrays with half as much again (at least 4096 records), rewrites thr and the device's walk array.  No record
// crosses PCIe and nothing is waited for BEFORE the launch: it is ordered behind the scatters that wrote the old arrays.
// The host waits once, for the kernel's end, before it releases the old arrays.  Nothing of the segment changes unless every
// allocation succeeded.
int univ3_make_room(cfmm_ctx* c, Segment& s, int64_t need)
{
    UniV3State& u = s.u;
    if (u.tick_used + need <= u.tick_cap) return CFMM_OK;
    constexpr int64_t kMaxRecords = 0x3fffffff / 2;   // the sweep's index arithmetic (univ3_build: 2·(T + 2m) <= 0x3fffffff)
    std::vector<int4> walk = u.h_walk;
    int64_t tight = 0;
    for (int4& w : walk) {   // a pool's two lists lie back to back: [x, x + y] and [z, z + w], z = x + y + 1
        const int base = (int)tight;
        tight += (int64_t)w.y + (int64_t)w.w + 2;
        w = make_int4(base, w.y, base + w.y + 1, w.w);
    }
    const int64_t want = tight + need;
    if (want > kMaxRecords) return fail(c, CFMM_ERR_UNSUPPORTED, "too many ticks in one segment");
    const int64_t cap = std::min(kMaxRecords, want + std::max<int64_t>(want / 2, 4096));
    DevBuf<TickRec> d_ticks;   // (the segment's own arrays stay until the launch is enqueued)
    DevBuf<double> d_thr;      // (the scan reads four thresholds at a time: + 4 behind the tail)
    DevBuf<int4> d_walk;
    if (d_ticks.alloc(c, (size_t)cap) != CFMM_OK || d_thr.alloc(c, (size_t)cap + 4) != CFMM_OK || d_walk.alloc(c, walk.size()) != CFMM_OK)
        return fail(c, CFMM_ERR_HIP, "pool update: allocation of %lld tick records failed", (long long)cap);
    UpdateStaging& st = c->upd;
    int rc = st.reserve(c, 2 * walk.size());
    if (rc != CFMM_OK) return rc;
    std::memcpy(st.buf.host(), walk.data(), walk.size() * sizeof(int4));
    const bool timed = c->opt_time_kernels != 0;
    for (Event& e : st.compact_ev)
        if (timed && (rc = e.create(c, hipEventDefault)) != CFMM_OK) return rc;
    HIP_TRY(c, launch_compact_walks(u.walk.get(), reinterpret_cast<const int4*>(st.buf.dev()), d_walk.get(), u.ticks.get(), d_ticks.get(), d_thr.get(),
                                    s.m, tight, c->stream, timed ? st.compact_ev[0].get() : nullptr, timed ? st.compact_ev[1].get() : nullptr));
    // One wait is kept, for the kernel itself: the old arrays are released below and the staging is refilled by the scatter that
    // follows, and both must outlive the kernel's reads (hipFree would wait for the device anyway; this says so).
    HIP_TRY(c, hipEventRecord(st.done.get(), c->stream));
    HIP_TRY(c, hipEventSynchronize(st.done.get()));
    st.busy = false;
    u.ticks = std::move(d_ticks);   // (releases the old arrays)
    u.thr = std::move(d_thr);
    u.walk = std::move(d_walk);
    c->desc_dirty = true;           // the sweep descriptors hold ticks / thr / walk
    u.h_walk.swap(walk);
    u.tick_used = tight;
    u.tick_cap = cap;
    ++c->pool_update_regrows;
    if (timed) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, st.compact_ev[0].get(), st.compact_ev[1].get()));
        st.compact_ns = (int64_t)((double)ms * 1e6);
    }
    return CFMM_OK;
}

int apply_univ3(cfmm_ctx* c, Segment& s, const Update& u, const Rows& rows)
{
    const int64_t k = (int64_t)rows.idx.size();
    // the moved pools' records, prepared as at upload (univ3_pool.h); list offsets relative to `ticks` until the tail is known
    std::vector<UniV3PoolRec> rec((size_t)k);
    std::vector<TickRec> ticks;
    std::vector<double> thr;
    bool fast = true, lists = false;
    const bool ladders = u.entry == kSetTicks;   // the rows bring their ladders; else the host's own (ladder_store.h)
    for (int64_t j = 0; j < k; ++j) {
        const int64_t i = rows.idx[(size_t)j], src = rows.src[(size_t)j];
        const int64_t nt = ladders ? u.tick_off[src + 1] - u.tick_off[src] : s.lad.count(i);
        const double* lt = ladders ? u.lt + u.tick_off[src] : s.lad.lower_ticks(i);
        const double* lq = ladders ? u.liq + u.tick_off[src] : s.lad.liquidity(i);
        const double cp = u.price[src];
        const int64_t ct = univ3_current_tick(lt, nt, cp);   // (>= 1: validated)
        univ3_prepare_pool(cp, s.h_gamma[(size_t)i], ct, nt, lt, lq, rec[(size_t)j], ticks);
        fast = fast && in_fast_window(cp) && (!ladders || univ3_liquidity_in_window(lq, nt));
        lists = lists || rec[(size_t)j].walk.y > 0 || rec[(size_t)j].walk.w > 0;
    }
    univ3_all_thresholds(ticks, thr);
    thr.resize(ticks.size() + 4, 0.0);
    const int64_t nrec = (int64_t)ticks.size();
    int rc = univ3_make_room(c, s, nrec);
    if (rc != CFMM_OK) return rc;
    UniV3State& st = s.u;
    // has_walk can only turn on: a segment uploaded without any list (no heads either) gets its heads now, all "never"
    DevBuf<uint4> new_head;
    if (!st.has_walk && lists && new_head.alloc(c, 2 * (size_t)s.m) != CFMM_OK)
        return fail(c, CFMM_ERR_HIP, "pool update: allocation of the threshold heads failed");
    const size_t words = (size_t)k * (2 + 1 + 2 + 2 + 1 + 2 + 2 + 4 + 1) + (size_t)nrec * 9 + 4;
    if ((rc = c->upd.reserve(c, words)) != CFMM_OK) return rc;
    if (new_head) {
        HIP_TRY(c, hipMemsetAsync(new_head.get(), 0, 2 * (size_t)s.m * sizeof(uint4), c->stream));
        st.head = std::move(new_head);
        st.has_walk = 1;
        c->desc_dirty = true;       // (the descriptors hold head and has_walk)
        c->geometry_dirty = true;   // (the plan reads has_walk: bytes per pool, hence "stream_stores" = auto)
    }
    const int base = (int)st.tick_used;
    Packer p(c);
    double2* pg = p.add<double2>(st.pg.get(), 2, k);
    double* cp = p.add<double>(st.cp.get(), 1, k);
    double2* cur_a = p.add<double2>(st.cur_a.get(), 2, k);
    double2* cur_b = p.add<double2>(st.cur_b.get(), 2, k);
    double* cur_c = p.add<double>(st.cur_c.get(), 1, k);
    double2* curR = p.add<double2>(st.curR.get(), 2, k);
    int4* walk = p.add<int4>(st.walk.get(), 2, k);
    uint4* head = st.head ? p.add<uint4>(st.head.get(), 4, k) : nullptr;
    TickRec* t_out = p.add<TickRec>(st.ticks.get(), 8, nrec, base);
    double* thr_out = p.add<double>(st.thr.get(), 1, nrec + 4, base);   // (+ the four read-ahead zeros behind the new tail)
    for (int64_t j = 0; j < k; ++j) {
        const UniV3PoolRec& r = rec[(size_t)j];
        pg[j] = r.pg;
        cp[j] = r.pg.x;
        cur_a[j] = r.cur_a;
        cur_b[j] = r.cur_b;
        cur_c[j] = r.cur_c;
        curR[j] = r.curR;
        if (head) univ3_heads(r.walk, thr.data(), head + 2 * j);
        walk[j] = make_int4(r.walk.x + base, r.walk.y, r.walk.z + base, r.walk.w);
    }
    std::memcpy(static_cast<void*>(t_out), ticks.data(), (size_t)nrec * sizeof(TickRec));
    std::memcpy(thr_out, thr.data(), ((size_t)nrec + 4) * sizeof(double));
    p.set_rows(rows.idx);
    if ((rc = launch(c, p)) != CFMM_OK) return rc;
    for (int64_t j = 0; j < k; ++j) {
        s.h_cp[(size_t)rows.idx[(size_t)j]] = rec[(size_t)j].pg.x;   // a later cfmm_update_reserves starts from the new prices
        st.h_walk[(size_t)rows.idx[(size_t)j]] = walk[j];
    }
    st.tick_used += nrec;
    if (!fast) s.fast_ok = 0;
    if (ladders) {   // the host's ladders follow; the plan reads n_ticks_total only through "more than 2 ticks per pool"
        const bool multi = s.n_ticks_total / s.m > 2;
        for (int64_t j = 0; j < k; ++j) {
            const int64_t src = rows.src[(size_t)j], o = u.tick_off[src];
            s.lad.replace(rows.idx[(size_t)j], u.tick_off[src + 1] - o, u.lt + o, u.liq + o);
        }
        s.n_ticks_total = s.lad.ticks_total();
        if ((s.n_ticks_total / s.m > 2) != multi) c->geometry_dirty = true;
    }
    return CFMM_OK;
}

int apply_reserves(cfmm_ctx* c, Segment& s, const Update& u, const Rows& rows)
{
    const int64_t k = (int64_t)rows.idx.size(), m = s.m;
    const bool ragged = ragged_kind(s.kind);
    const int nc = ragged ? s.n_coins : 2;
    int rc = c->upd.reserve(c, (size_t)k * (2 * (size_t)nc + 2 + 1));
    if (rc != CFMM_OK) return rc;
    Packer p(c);
    bool fast = true;
    if (!ragged) {
        double2* R = p.add<double2>(s.R.get(), 2, k);
        double2* Q = s.kind == CFMM_KIND_GEOMEAN ? p.add<double2>(s.lR.get(), 2, k) : nullptr;
        for (int64_t j = 0; j < k; ++j) {
            const double* r = u.R + 2 * rows.src[(size_t)j];
            const size_t i = (size_t)rows.idx[(size_t)j];
            R[j] = make_double2(r[0], r[1]);
            fast = fast && in_fast_window(r[0]) && in_fast_window(r[1]);
            if (Q) Q[j] = geomean_q(s.h_gamma[i], s.h_eta[i], r[0], r[1]);
        }
    } else {
        // coin-major columns: one staging column per coin
        double *R[kMaxCoins], *q[kMaxCoins];
        for (int c2 = 0; c2 < nc; ++c2) R[c2] = p.add<double>(s.nc.R.get() + (size_t)c2 * (size_t)m, 1, k);
        for (int c2 = 0; c2 < nc; ++c2) q[c2] = p.add<double>(s.nc.q.get() + (size_t)c2 * (size_t)m, 1, k);
        double2* ab = s.kind == CFMM_KIND_CURVE ? p.add<double2>(s.nc.par.get(), 2, k) : nullptr;
        for (int64_t j = 0; j < k; ++j) {
            const int64_t src = rows.src[(size_t)j];
            const double* r = u.R + nc * src;
            const size_t i = (size_t)rows.idx[(size_t)j];
            double qq[kMaxCoins], par[2];
            if (ab) {
                curve_fill(r, u.alpha[src], u.beta[src], nc, qq, par);
                ab[j] = make_double2(par[0], par[1]);
            } else {
                for (int c2 = 0; c2 < nc; ++c2) qq[c2] = weighted_q(r[c2], s.h_par[(size_t)c2 * (size_t)m + i]);
            }
            for (int c2 = 0; c2 < nc; ++c2) {
                R[c2][j] = r[c2];
                q[c2][j] = qq[c2];
            }
        }
    }
    p.set_rows(rows.idx);
    if ((rc = launch(c, p)) != CFMM_OK) return rc;
    if (!fast) s.fast_ok = 0;   // (the kinds with one arithmetic have fast_ok = 0 already)
    return CFMM_OK;
}

// One validated update on a single-device context
int apply(cfmm_ctx* c, const Update& u)
{
    if (u.count == 0) return CFMM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    armed_cancel(c);
    Segment& s = c->segs[(size_t)u.seg];
    const Rows rows = distinct_rows(u.count, u.idx);
    const int rc = univ3_entry(u.entry) ? apply_univ3(c, s, u, rows) : apply_reserves(c, s, u, rows);
    if (rc != CFMM_OK) return rc;
    // as cfmm_update_reserves: the trades and outputs on the device describe the market before the update
    c->have_trades = false;
    c->have_out = false;
    c->x_valid = false;
    c->trade_v.clear();
    return CFMM_OK;
}

// Multi-device parents: the rows split by shard_range, every shard's part checked before any shard changes
int multi_update(cfmm_ctx* c, const Update& u)
{
    int rc = check_args(c, u, (int64_t)c->psegs.size());
    if (rc != CFMM_OK) return rc;
    const auto& ps = c->psegs[(size_t)u.seg];
    if ((rc = check_entry(c, u.entry, ps.kind)) != CFMM_OK || (rc = check_arrays(c, u)) != CFMM_OK) return rc;
    if (u.count == 0) return CFMM_OK;
    const int nd = (int)c->shards.size(), nc = ps.n_coins;
    struct Part {
        std::vector<int64_t> idx;
        std::vector<double> R, alpha, beta, price, lt, liq;
        std::vector<int64_t> tick_off;
        int64_t lo = 0;
        Update u{};
    };
    std::vector<Part> parts((size_t)nd);
    std::vector<int64_t> los((size_t)nd), his((size_t)nd);
    for (int d = 0; d < nd; ++d) shard_range(ps.m, d, nd, los[(size_t)d], his[(size_t)d]);
    for (int64_t j = 0; j < u.count; ++j) {
        const int64_t i = u.idx[j];
        if (i < 0 || i >= ps.m) return fail(c, CFMM_ERR_INVALID_ARG, "pool index %lld out of range [0, %lld)", (long long)i, (long long)ps.m);
        int d = 0;
        while (i >= his[(size_t)d]) ++d;
        Part& p = parts[(size_t)d];
        p.idx.push_back(i - los[(size_t)d]);
        if (univ3_entry(u.entry)) p.price.push_back(u.price[j]);
        if (u.entry == kSetTicks) {   // the shard's own CSR; offsets that run backwards become an empty ladder ("needs at least one tick")
            const int64_t o = u.tick_off[j], nt = o >= 0 && u.tick_off[j + 1] > o ? u.tick_off[j + 1] - o : 0;
            if (p.tick_off.empty()) p.tick_off.push_back(0);
            p.lt.insert(p.lt.end(), u.lt + o, u.lt + o + nt);
            p.liq.insert(p.liq.end(), u.liq + o, u.liq + o + nt);
            p.tick_off.push_back((int64_t)p.lt.size());
        }
        if (!univ3_entry(u.entry)) p.R.insert(p.R.end(), u.R + j * nc, u.R + (j + 1) * nc);
        if (u.entry == kSetCurve) {
            p.alpha.push_back(u.alpha[j]);
            p.beta.push_back(u.beta[j]);
        }
    }
    for (int d = 0; d < nd; ++d) {
        Part& p = parts[(size_t)d];
        p.lo = los[(size_t)d];
        p.u = Update{u.entry, (int32_t)child_segment(c, u.seg, d), (int64_t)p.idx.size(), p.idx.data(), p.R.data(), p.alpha.data(),
                     p.beta.data(), p.price.data(), p.tick_off.data(), p.lt.data(), p.liq.data()};
        if (u.entry == kSetTicks && p.lt.empty()) p.u.lt = p.u.liq = &kNoTick;   // (rows without a tick: refused by row, not as a null array)
        if (p.idx.empty()) continue;
        cfmm_ctx* child = c->shards[(size_t)d];
        if ((rc = validate(child, p.u, p.lo)) != CFMM_OK) return fail(c, rc, "%s", child->err.c_str());
    }
    for (int d = 0; d < nd; ++d) {
        Part& p = parts[(size_t)d];
        if (p.idx.empty()) continue;
        cfmm_ctx* child = c->shards[(size_t)d];
        if ((rc = apply(child, p.u)) != CFMM_OK) {
            c->have_trades = c->have_out = false;   // some shards may have moved
            return fail(c, rc, "shard %d: %s", d, child->err.c_str());
        }
    }
    c->have_trades = c->have_out = false;
    return CFMM_OK;
}

int update(cfmm_ctx* c, const Update& u)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) return multi_update(c, u);
    const int rc = validate(c, u, 0);
    return rc != CFMM_OK ? rc : apply(c, u);
}

} // namespace

int cfmm::univ3_move_prices(cfmm_ctx* c, Segment& s, const std::vector<int64_t>& rows, const double* price)
{
    if (rows.empty()) return CFMM_OK;
    Rows r;
    r.idx = rows;
    r.src.resize(rows.size());
    for (size_t k = 0; k < rows.size(); ++k) r.src[k] = (int64_t)k;
    return apply_univ3(c, s, Update{kSetPrices, 0, (int64_t)rows.size(), rows.data(), nullptr, nullptr, nullptr, price, nullptr, nullptr, nullptr}, r);
}

// The staging buffer with room for `words` 8-byte words, free for the host to fill: the previous scatter has read it
int cfmm::UpdateStaging::reserve(cfmm_ctx* c, size_t words)
{
    if (busy) {
        HIP_TRY(c, hipEventSynchronize(done.get()));
        busy = false;
    }
    if (const int rc = done.create(c, hipEventDisableTiming)) return rc;
    words += 8 * (size_t)kMaxScatterCols;   // (+ the columns' alignment)
    if (words <= buf.size()) return CFMM_OK;
    size_t cap = std::max<size_t>(buf.size() * 2, 1 << 13);
    while (cap < words) cap *= 2;
    if (buf.alloc(c, cap, true) != CFMM_OK || !buf.dev()) {
        buf.reset();
        return fail(c, CFMM_ERR_HIP, "pool update: staging allocation of %zu bytes failed", cap * 8);
    }
    return CFMM_OK;
}

extern "C" {

int cfmm_pools_set_reserves(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const double* R)
{
    return update(c, Update{kSetReserves, seg, count, idx, R, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
}

int cfmm_pools_set_curve(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const double* R, const double* alpha,
                         const double* beta)
{
    return update(c, Update{kSetCurve, seg, count, idx, R, alpha, beta, nullptr, nullptr, nullptr, nullptr});
}

int cfmm_pools_set_prices(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const double* current_price)
{
    return update(c, Update{kSetPrices, seg, count, idx, nullptr, nullptr, nullptr, current_price, nullptr, nullptr, nullptr});
}

int cfmm_pools_set_ticks(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const double* current_price,
                         const int64_t* tick_off, const double* lower_ticks, const double* liquidity)
{
    return update(c, Update{kSetTicks, seg, count, idx, nullptr, nullptr, nullptr, current_price, tick_off, lower_ticks, liquidity});
}

} // extern "C"
