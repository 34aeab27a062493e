// abi_find_path.cpp -- cfmm_find_path: the best swap walk of at most max_hops hops between two tokens, found on the device by
// layers (the kernels and the contract: find_path_kernels.h; the checks and the chunking rule: find_checks.h).
// Read-only.  Like the path quotes the kernels see the segments through a table in device memory (sweep.h FindSeg) that
// build_find_table below REBUILDS FROM THE SEGMENTS' CURRENT ADDRESSES (seg_view.h) AND UPLOADS ON EVERY CALL: it is never a cache.
// The queries are processed in chunks whose layers fit kFindScratchBudget; a chunk is a sequence of launches on the context's
// stream -- clear, find_init, find_relax per layer, find_select, then find_claim + find_advance per layer from the last, and
// find_finish, which writes the chunk's part of the call's outputs -- and no chunk reads what another wrote, so the results do
// not depend on the chunking.  One synchronisation, at the end.
// cfmm_find_path_out (include/cfmm_amd_find_out.h) is the same call in the other direction, as abi_swap_path.cpp serves both path
// executions: the same table, staging, chunks and timing, the kFindOut* kernels, the layers cleared to all ones (the unreached
// word of a min-search) and the two amounts exchanged -- FindArgs::amount_in carries the wanted amount_out.
// cfmm_find_disjoint_paths (include/cfmm_amd_find_disjoint.h) is the exact-input search run max_paths times per chunk with the
// kernels that know the ban (find_disjoint_kernels.h): the same table, staging, chunks (find_disjoint_chunk_queries: the ban row
// counts) and timing, the outputs one dimension larger, round r's finish writing slot r.  cfmm_find_disjoint_paths_out
// (include/cfmm_amd_find_disjoint_out.h) is that call in the other direction, by the Direction find_paths takes: the backwards
// kernels of each role, the layers cleared to all ones, the none value of cfmm_find_path_out.
#include "find_checks.h"
#include "seg_view.h"
#include "stage_layout.h"
#include "../../include/cfmm_amd_find_disjoint.h"
#include "../../include/cfmm_amd_find_disjoint_out.h"
#include "../../include/cfmm_amd_find_out.h"

#include <algorithm>
#include <cstring>

using namespace cfmm;

namespace {

// the two directions: the entry's name, the given amount's name in a refusal, what a query without a path answers
struct Direction {
    bool out;
    const char* who;
    const char* amount;
    FindKernel kernel(FindKernel k) const { return out ? (FindKernel)(k + kFindOutFirst) : k; }
    // exact input: 0.0.  exact output: +inf, cfmm_quote_out's "cannot give that much" -- but buying nothing costs nothing
    double none(double given) const { return !out || given == 0.0 ? 0.0 : __builtin_inf(); }
};
constexpr Direction kExactIn{false, "cfmm_find_path", "amount_in"}, kExactOut{true, "cfmm_find_path_out", "amount_out"};
constexpr Direction kDisjointIn{false, "cfmm_find_disjoint_paths", "amount_in"}, kDisjointOut{true, "cfmm_find_disjoint_paths_out", "amount_out"};

// one record per segment (seg_view.h: from the addresses the segment holds NOW; every stored segment has pools); returns the
// blocks that cover them (and, where asked, the pools: the numbers an edge and a ban bit carry run below it)
int64_t build_find_table(const cfmm_ctx* c, FindSeg* t, int64_t* n_pools = nullptr)
{
    int64_t tiles = 0, pools = 0;
    build_table(c, t, [&](const Segment& s, size_t) {
        const FindSeg f = find_seg(s, tiles, pools);
        tiles += (s.m + kFindBlock - 1) / kFindBlock;
        pools += s.m;
        return f;
    });
    if (n_pools) *n_pools = pools;
    return tiles;
}

struct Timing {
    bool on;
    std::vector<int> what, layer, round;   // FindKernel, layer and round of every timed launch, in order: launch k has pair k of FindScratch::ev
};

// ban: cfmm_find_disjoint_paths' kernel of the same role (launch_find_ban); round: the round the launch's span is booked to
int launch(cfmm_ctx* c, Timing& t, FindKernel k, const FindArgs& a, const FindBanArgs* ban = nullptr, int round = 0)
{
    EventPairs& ev = c->find.ev;
    const size_t j = t.what.size();
    if (t.on) {
        const int rc = ev.ensure(c, j + 1, j);
        if (rc != CFMM_OK) return rc;
        t.what.push_back(k);
        t.layer.push_back(a.layer);
        t.round.push_back(round);
    }
    const hipError_t e = ban ? launch_find_ban(k, a, *ban, c->stream, ev.start(j, t.on), ev.stop(j, t.on))
                             : launch_find(k, a, c->stream, ev.start(j, t.on), ev.stop(j, t.on));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "find path launch failed: %s", hipGetErrorString(e));
    ++c->find.launches;
    return CFMM_OK;
}

void clear_times(FindScratch& fs)
{
    fs.launches = fs.relax_ns = fs.walk_ns = 0;
    std::memset(fs.layer_ns, 0, sizeof fs.layer_ns);
    std::memset(fs.round_ns, 0, sizeof fs.round_ns);
}

// the timed launches' spans into the read-only options (behind the call's synchronisation)
int collect_times(cfmm_ctx* c, const Timing& timing)
{
    FindScratch& fs = c->find;
    for (size_t k = 0; k < timing.what.size(); ++k) {
        int64_t ns = 0;
        const int rc = fs.ev.elapsed_ns(c, k, 1, ns);
        if (rc != CFMM_OK) return rc;
        const int w = timing.what[k] >= kFindOutFirst ? timing.what[k] - kFindOutFirst : timing.what[k], h = timing.layer[k];
        const bool walk = w == kFindClaim || w == kFindAdvance;
        if (w == kFindRelax) fs.relax_ns += ns;
        if (walk) fs.walk_ns += ns;
        if ((w == kFindRelax || walk) && h >= 1 && h <= CFMM_MAX_PATH_HOPS)
            fs.layer_ns[w == kFindRelax ? 0 : (w == kFindClaim ? 1 : 2)][h - 1] += ns;
        if (w == kFindRelax || walk) fs.round_ns[walk][timing.round[k]] += ns;
    }
    return CFMM_OK;
}

// the LDS copy of the layer launches for a chunk of cq queries (option "find_lds", default on): where a group of queries' rows
// fit it, a block folding enough tiles that about four blocks per CU remain
void set_lds_group(const cfmm_ctx* c, FindArgs& a, size_t cq, int64_t tiles)
{
    a.group = c->opt_find_lds != 0 ? find_lds_group(c->n) : 0;
    if (a.group > 0) {
        a.group = (int32_t)std::min<int64_t>(a.group, (int64_t)cq);
        const int64_t rows = ((int64_t)cq + a.group - 1) / a.group;
        a.tiles_per_block = (int32_t)std::clamp<int64_t>(tiles * rows / 1024, 1, 64);
        if (rows > 65535) a.group = 0;
    }
}

// both entries; amount_in is the GIVEN amount and amount_out the ANSWER, whichever side of the path each stands on
int find_paths(const Direction& d, cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
               const double* amount_in, double* amount_out, int32_t* n_hops, int32_t* hop_seg, int64_t* hop_row,
               int32_t* hop_coin_in, int32_t* hop_coin_out, int32_t* status)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const char* const kWho = d.who;
    if (is_parent(c))
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context: the layers of the search live on one "
                                             "device (find on a single-device context of the same pools)", kWho);
    char msg[256] = "";
    int rc = check_find(kWho, c->n, count, max_hops, token_in, token_out, amount_in, amount_out, n_hops, hop_seg, hop_row, hop_coin_in,
                        hop_coin_out, status, msg, sizeof msg, d.amount);
    if (rc != CFMM_OK) return fail(c, rc, "%s", msg);
    if (count == 0) return CFMM_OK;
    FindScratch& fs = c->find;
    clear_times(fs);
    const size_t n = (size_t)count, H = (size_t)max_hops, nh = n * H;
    if (c->segs.empty()) {   // a market without pools reaches nothing
        for (size_t q = 0; q < n; ++q) {
            amount_out[q] = d.none(amount_in[q]);
            n_hops[q] = 0;
            status[q] = CFMM_FOUND_NONE;
        }
        for (size_t at = 0; at < nh; ++at) {
            hop_seg[at] = hop_coin_in[at] = hop_coin_out[at] = -1;
            hop_row[at] = -1;
        }
        return CFMM_OK;
    }

    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nseg = c->segs.size(), nt = (size_t)c->n;
    const size_t chunk = (size_t)std::min<int64_t>(count, find_chunk_queries(c->n, max_hops));
    const FindStage lay(nseg * sizeof(FindSeg), n, nh);   // the pinned staging (stage_layout.h)
    if ((rc = fs.stage.grow(c, lay.l.words(), false)) || (rc = fs.table.grow(c, nseg)) || (rc = fs.best.grow(c, (H + 1) * chunk * nt)) ||
        (rc = fs.edge.grow(c, H * chunk)) || (rc = fs.i32.grow(c, 4 * n + 3 * nh + 2 * chunk)) || (rc = fs.hop_row.grow(c, nh)) ||
        (rc = fs.amt.grow(c, 2 * n)))
        return rc;
    unsigned long long* st = fs.stage.host();
    FindSeg* h_table = reinterpret_cast<FindSeg*>(lay.table.in(st));
    const int64_t tiles = build_find_table(c, h_table);
    int32_t *h_tok = lay.tok.in(st), *h_ns = lay.ns.in(st), *h_hop32 = lay.hop32.in(st);
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st);
    long long* h_row = lay.row.in(st);
    std::memcpy(h_tok, token_in, n * sizeof(int32_t));
    std::memcpy(h_tok + n, token_out, n * sizeof(int32_t));
    std::memcpy(h_amt, amount_in, n * sizeof(double));
    int32_t* d_i32 = fs.i32.get();
    HIP_TRY(c, hipMemcpyAsync(fs.table.get(), h_table, nseg * sizeof(FindSeg), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_i32, h_tok, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(fs.amt.get(), h_amt, n * sizeof(double), hipMemcpyHostToDevice, c->stream));

    Timing timing{c->opt_time_kernels != 0, {}, {}, {}};
    for (size_t q0 = 0; q0 < n; q0 += chunk) {
        const size_t cq = std::min(chunk, n - q0);
        FindArgs a{};
        a.count = (int64_t)cq;
        a.stride = count;
        a.max_hops = max_hops;
        a.nseg = (int32_t)nseg;
        a.n_tokens = c->n;
        a.tiles = tiles;
        a.segs = fs.table.get();
        a.token_in = d_i32 + q0;
        a.token_out = d_i32 + n + q0;
        a.n_hops = d_i32 + 2 * n + q0;
        a.status = d_i32 + 3 * n + q0;
        a.hop_seg = d_i32 + 4 * n + q0;
        a.hop_coin_in = d_i32 + 4 * n + nh + q0;
        a.hop_coin_out = d_i32 + 4 * n + 2 * nh + q0;
        a.h_star = d_i32 + 4 * n + 3 * nh;
        a.target = d_i32 + 4 * n + 3 * nh + chunk;
        a.hop_row = fs.hop_row.get() + q0;
        a.amount_in = fs.amt.get() + q0;
        a.amount_out = fs.amt.get() + n + q0;
        a.best = fs.best.get();
        a.edge = fs.edge.get();
        HIP_TRY(c, hipMemsetAsync(a.best, d.out ? 0xff : 0, (H + 1) * cq * nt * sizeof(unsigned long long), c->stream));
        HIP_TRY(c, hipMemsetAsync(a.edge, 0xff, H * cq * sizeof(unsigned long long), c->stream));
        if ((rc = launch(c, timing, d.kernel(kFindInit), a)) != CFMM_OK) return rc;
        set_lds_group(c, a, cq, tiles);   // the layers
        for (a.layer = 1; a.layer <= max_hops; ++a.layer)
            if ((rc = launch(c, timing, d.kernel(kFindRelax), a)) != CFMM_OK) return rc;
        a.group = 0;
        if ((rc = launch(c, timing, d.kernel(kFindSelect), a)) != CFMM_OK) return rc;
        for (a.layer = max_hops; a.layer >= 1; --a.layer)
            if ((rc = launch(c, timing, d.kernel(kFindClaim), a)) || (rc = launch(c, timing, d.kernel(kFindAdvance), a))) return rc;
        a.layer = 0;
        if ((rc = launch(c, timing, d.kernel(kFindFinish), a)) != CFMM_OK) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(h_out, fs.amt.get() + n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_ns, d_i32 + 2 * n, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_hop32, d_i32 + 4 * n, 3 * nh * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_row, fs.hop_row.get(), nh * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = collect_times(c, timing)) != CFMM_OK) return rc;
    std::memcpy(amount_out, h_out, n * sizeof(double));
    std::memcpy(n_hops, h_ns, n * sizeof(int32_t));
    std::memcpy(status, h_ns + n, n * sizeof(int32_t));
    std::memcpy(hop_seg, h_hop32, nh * sizeof(int32_t));
    std::memcpy(hop_coin_in, h_hop32 + nh, nh * sizeof(int32_t));
    std::memcpy(hop_coin_out, h_hop32 + 2 * nh, nh * sizeof(int32_t));
    std::memcpy(hop_row, h_row, nh * sizeof(long long));
    return CFMM_OK;
}

// cfmm_find_disjoint_paths / cfmm_find_disjoint_paths_out: find_paths' table, staging, chunks and timing; per chunk the ban rows
// are cleared once and max_paths rounds follow, each the launches of one search of the direction with the kernels that know
// the ban, its finish writing slot r.  As in find_paths amount_in is the GIVEN amount and amount_out the ANSWER.
int find_disjoint(const Direction& d, cfmm_ctx* c, int64_t count, int32_t max_paths, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                  const double* amount_in, int32_t* n_paths, double* amount_out, int32_t* n_hops, int32_t* status, int32_t* hop_seg,
                  int64_t* hop_row, int32_t* hop_coin_in, int32_t* hop_coin_out)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const char* const kWho = d.who;
    if (is_parent(c))
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context: the layers of the search live on one "
                                             "device (find on a single-device context of the same pools)", kWho);
    char msg[256] = "";
    int rc = check_find_disjoint(kWho, c->n, count, max_paths, max_hops, token_in, token_out, amount_in, n_paths, amount_out, n_hops, status,
                                 hop_seg, hop_row, hop_coin_in, hop_coin_out, msg, sizeof msg, d.amount);
    if (rc != CFMM_OK) return fail(c, rc, "%s", msg);
    if (count == 0) return CFMM_OK;
    FindScratch& fs = c->find;
    clear_times(fs);
    const size_t n = (size_t)count, H = (size_t)max_hops, K = (size_t)max_paths, nh = n * H;
    if (c->segs.empty()) {   // a market without pools reaches nothing
        std::fill(n_paths, n_paths + n, 0);
        for (size_t r = 0; r < K; ++r)
            for (size_t q = 0; q < n; ++q) amount_out[r * n + q] = d.none(amount_in[q]);
        std::fill(n_hops, n_hops + K * n, 0);
        std::fill(status, status + K * n, CFMM_FOUND_NONE);
        std::fill(hop_seg, hop_seg + K * nh, -1);
        std::fill(hop_row, hop_row + K * nh, (int64_t)-1);
        std::fill(hop_coin_in, hop_coin_in + K * nh, -1);
        std::fill(hop_coin_out, hop_coin_out + K * nh, -1);
        return CFMM_OK;
    }

    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nseg = c->segs.size(), nt = (size_t)c->n;
    const FindDisjointStage lay(nseg * sizeof(FindSeg), n, K, nh);   // the pinned staging (stage_layout.h)
    if ((rc = fs.stage.grow(c, lay.l.words(), false)) != CFMM_OK) return rc;
    unsigned long long* st = fs.stage.host();
    FindSeg* h_table = reinterpret_cast<FindSeg*>(lay.table.in(st));
    int64_t pools = 0;   // of the table: every pool number an edge or a ban bit carries is below it
    const int64_t tiles = build_find_table(c, h_table, &pools);
    const size_t bw = (size_t)find_ban_words(pools);
    const size_t chunk = (size_t)std::min<int64_t>(count, find_disjoint_chunk_queries(c->n, max_hops, pools));
    // FindScratch::i32: [3][n] token_in, token_out, n_paths; [2][K][n] n_hops, status; [3][K][H][n] the int32 hop arrays; [3][chunk]
    if ((rc = fs.table.grow(c, nseg)) || (rc = fs.best.grow(c, (H + 1) * chunk * nt)) || (rc = fs.edge.grow(c, H * chunk)) ||
        (rc = fs.i32.grow(c, 3 * n + 2 * K * n + 3 * K * nh + 3 * chunk)) || (rc = fs.hop_row.grow(c, K * nh)) ||
        (rc = fs.amt.grow(c, n + K * n)) || (rc = fs.ban.grow(c, chunk * bw)))
        return rc;
    int32_t *h_tok = lay.tok.in(st), *h_ns = lay.ns.in(st), *h_hop32 = lay.hop32.in(st);
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st);
    long long* h_row = lay.row.in(st);
    std::memcpy(h_tok, token_in, n * sizeof(int32_t));
    std::memcpy(h_tok + n, token_out, n * sizeof(int32_t));
    std::memcpy(h_amt, amount_in, n * sizeof(double));
    int32_t* d_i32 = fs.i32.get();
    int32_t *d_np = d_i32 + 2 * n, *d_nh = d_np + n, *d_st = d_nh + K * n, *d_hop = d_st + K * n, *d_chunk = d_hop + 3 * K * nh;
    HIP_TRY(c, hipMemcpyAsync(fs.table.get(), h_table, nseg * sizeof(FindSeg), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_i32, h_tok, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(fs.amt.get(), h_amt, n * sizeof(double), hipMemcpyHostToDevice, c->stream));

    Timing timing{c->opt_time_kernels != 0, {}, {}, {}};
    for (size_t q0 = 0; q0 < n; q0 += chunk) {
        const size_t cq = std::min(chunk, n - q0);
        FindArgs a{};
        a.count = (int64_t)cq;
        a.stride = count;
        a.max_hops = max_hops;
        a.nseg = (int32_t)nseg;
        a.n_tokens = c->n;
        a.tiles = tiles;
        a.segs = fs.table.get();
        a.token_in = d_i32 + q0;
        a.token_out = d_i32 + n + q0;
        a.h_star = d_chunk;
        a.target = d_chunk + chunk;
        a.amount_in = fs.amt.get() + q0;
        a.best = fs.best.get();
        a.edge = fs.edge.get();
        FindBanArgs b{};
        b.ban = fs.ban.get();          // indexed by the CHUNK's query number, cleared per chunk
        b.ban_words = (int64_t)bw;
        b.ended = d_chunk + 2 * chunk;
        b.n_paths = d_np + q0;
        HIP_TRY(c, hipMemsetAsync(b.ban, 0, cq * bw * sizeof(unsigned long long), c->stream));
        for (size_t r = 0; r < K; ++r) {
            const int round = b.round = (int32_t)r;
            a.n_hops = d_nh + r * n + q0;          // slot r of the outputs
            a.status = d_st + r * n + q0;
            a.amount_out = fs.amt.get() + n + r * n + q0;
            a.hop_seg = d_hop + r * nh + q0;
            a.hop_coin_in = d_hop + (K + r) * nh + q0;
            a.hop_coin_out = d_hop + (2 * K + r) * nh + q0;
            a.hop_row = fs.hop_row.get() + r * nh + q0;
            a.layer = 0;
            a.group = 0;
            HIP_TRY(c, hipMemsetAsync(a.best, d.out ? 0xff : 0, (H + 1) * cq * nt * sizeof(unsigned long long), c->stream));
            HIP_TRY(c, hipMemsetAsync(a.edge, 0xff, H * cq * sizeof(unsigned long long), c->stream));
            if ((rc = launch(c, timing, d.kernel(kFindInit), a, &b, round)) != CFMM_OK) return rc;
            set_lds_group(c, a, cq, tiles);
            for (a.layer = 1; a.layer <= max_hops; ++a.layer)
                if ((rc = launch(c, timing, d.kernel(kFindRelax), a, &b, round)) != CFMM_OK) return rc;
            a.group = 0;
            if ((rc = launch(c, timing, d.kernel(kFindSelect), a, nullptr, round)) != CFMM_OK) return rc;
            for (a.layer = max_hops; a.layer >= 1; --a.layer)
                if ((rc = launch(c, timing, d.kernel(kFindClaim), a, &b, round)) || (rc = launch(c, timing, d.kernel(kFindAdvance), a, nullptr, round)))
                    return rc;
            a.layer = 0;
            if ((rc = launch(c, timing, d.kernel(kFindFinish), a, &b, round)) != CFMM_OK) return rc;
        }
    }
    HIP_TRY(c, hipMemcpyAsync(h_out, fs.amt.get() + n, K * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_ns, d_np, (n + 2 * K * n) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_hop32, d_hop, 3 * K * nh * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_row, fs.hop_row.get(), K * nh * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = collect_times(c, timing)) != CFMM_OK) return rc;
    std::memcpy(amount_out, h_out, K * n * sizeof(double));
    std::memcpy(n_paths, h_ns, n * sizeof(int32_t));
    std::memcpy(n_hops, h_ns + n, K * n * sizeof(int32_t));
    std::memcpy(status, h_ns + n + K * n, K * n * sizeof(int32_t));
    std::memcpy(hop_seg, h_hop32, K * nh * sizeof(int32_t));
    std::memcpy(hop_coin_in, h_hop32 + K * nh, K * nh * sizeof(int32_t));
    std::memcpy(hop_coin_out, h_hop32 + 2 * K * nh, K * nh * sizeof(int32_t));
    std::memcpy(hop_row, h_row, K * nh * sizeof(long long));
    return CFMM_OK;
}

} // namespace

int cfmm_find_disjoint_paths(cfmm_ctx* c, int64_t count, int32_t max_paths, int32_t max_hops, const int32_t* token_in,
                             const int32_t* token_out, const double* amount_in, int32_t* n_paths, double* amount_out,
                             int32_t* n_hops, int32_t* status, int32_t* hop_seg, int64_t* hop_row, int32_t* hop_coin_in,
                             int32_t* hop_coin_out)
{
    return find_disjoint(kDisjointIn, c, count, max_paths, max_hops, token_in, token_out, amount_in, n_paths, amount_out, n_hops, status, hop_seg,
                         hop_row, hop_coin_in, hop_coin_out);
}

int cfmm_find_disjoint_paths_out(cfmm_ctx* c, int64_t count, int32_t max_paths, int32_t max_hops, const int32_t* token_in,
                                 const int32_t* token_out, const double* amount_out, int32_t* n_paths, double* amount_in,
                                 int32_t* n_hops, int32_t* status, int32_t* hop_seg, int64_t* hop_row, int32_t* hop_coin_in,
                                 int32_t* hop_coin_out)
{
    return find_disjoint(kDisjointOut, c, count, max_paths, max_hops, token_in, token_out, amount_out, n_paths, amount_in, n_hops, status,
                         hop_seg, hop_row, hop_coin_in, hop_coin_out);
}

int cfmm_find_path(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                   const double* amount_in, double* amount_out, int32_t* n_hops, int32_t* hop_seg, int64_t* hop_row,
                   int32_t* hop_coin_in, int32_t* hop_coin_out, int32_t* status)
{
    return find_paths(kExactIn, c, count, max_hops, token_in, token_out, amount_in, amount_out, n_hops, hop_seg, hop_row, hop_coin_in,
                      hop_coin_out, status);
}

int cfmm_find_path_out(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                       const double* amount_out, double* amount_in, int32_t* n_hops, int32_t* hop_seg, int64_t* hop_row,
                       int32_t* hop_coin_in, int32_t* hop_coin_out, int32_t* status)
{
    return find_paths(kExactOut, c, count, max_hops, token_in, token_out, amount_out, amount_in, n_hops, hop_seg, hop_row, hop_coin_in,
                      hop_coin_out, status);
}
