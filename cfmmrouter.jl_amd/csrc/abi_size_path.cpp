// abi_size_path.cpp -- cfmm_size_path / cfmm_size_path_dev (include/cfmm_amd_size_path.h): the input of a path that maximises its
// gain, by a bracketing search of rounds x 64 trial sizes in ONE launch, one wavefront per path (the kernel:
// size_path_kernels.h; the search's arithmetic: size_grid.h, shared with it; the checks: size_checks.h and path_checks.h).
// Read-only.  As in abi_quote_path.cpp the kernel sees the segments through a table of PathSeg records in device memory,
// rebuilt and uploaded on every call by the rig of the read-only path entries (ctx.h TimedPathRig, path_rig.h).
// The only memory of the feature is SizeScratch (ctx.h): proportional to count x max_hops, never to the pools.
// A multi-device parent runs the search on the host (multi_size): per round one cfmm_quote_path call of 64 x count paths
// through the parent path, the trial sizes, gains and selection by size_grid.h -- the text the kernel compiles -- so the
// answers are the same bits.
#include "path_rig.h"
#include "size_checks.h"
#include "split_search.h"
#include "stage_layout.h"

#include <cstring>
#include <vector>

using namespace cfmm;

namespace {

constexpr const char* kWho = "cfmm_size_path";
constexpr const char* kWhoDev = "cfmm_size_path_dev";

SizeStage stage_of(const cfmm_ctx* c, size_t n, size_t nh) { return SizeStage(table_records(c) * sizeof(PathSeg), n, nh); }

int launch(cfmm_ctx* c, const SizeArgs& a)
{
    SizeScratch& sc = c->size;
    const int rc = sc.launch(c, sc.ev, "size path",
                             [&](hipEvent_t e0, hipEvent_t e1) { return launch_size_path(a, c->opt_size_max_blocks, c->stream, e0, e1); });
    if (rc == CFMM_OK) sc.launches = 1;
    return rc;
}

// A parent.  Per round the 64 trial sizes of every path (trial j of path p is path j*count + p of the inner call: split_search.h
// GridPaths) go through cfmm_quote_path's parent path; the rest is size_grid.h.  Everything was checked by the caller; the
// answers are written only when every call has succeeded.
int multi_size(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
               const int32_t* ci, const int32_t* co, const double* max_in, const double* value_in, const double* value_out,
               int32_t rounds, double* amount_in, double* amount_out, double* gain, int32_t* status)
{
    constexpr size_t J = CFMM_SIZE_POINTS;
    const size_t n = (size_t)count, N = J * n;
    const GridPaths gp(count, max_hops, n_hops, hop_seg, hop_row, ci, co);
    std::vector<double> lo(n, 0.0), hi(max_in, max_in + n), x(N), y(N), bx(n, 0.0), by(n, 0.0), bg(n, 0.0);
    std::vector<char> any_nan(n, 0);
    SizeScratch& sc = c->size;
    int64_t ns = 0;
    for (int r = 0; r < rounds; ++r) {
        for (size_t j = 0; j < J; ++j)
            for (size_t p = 0; p < n; ++p) x[j * n + p] = size_trial(lo[p], hi[p], (int)j);
        const int rc = cfmm_quote_path(c, (int64_t)N, max_hops, gp.nh.data(), gp.seg.data(), gp.row.data(), gp.cin.data(), gp.cot.data(),
                                       x.data(), y.data(), nullptr);
        if (rc != CFMM_OK) return rc;   // (the message is the inner call's)
        if (c->opt_time_kernels != 0) ns += c->quote.ns;
        for (size_t p = 0; p < n; ++p) {
            const double vi = value_in ? value_in[p] : 1.0, vo = value_out ? value_out[p] : 1.0;
            int bj = 0;
            double g = size_gain(vi, vo, x[p], y[p]);
            for (size_t j = 1; j < J; ++j) {
                const double gj = size_gain(vi, vo, x[j * n + p], y[j * n + p]);
                if (size_better(gj, (int)j, g, bj)) {
                    g = gj;
                    bj = (int)j;
                }
            }
            any_nan[p] = any_nan[p] || g != g;
            lo[p] = x[(size_t)size_left(bj) * n + p];
            hi[p] = x[(size_t)size_right(bj) * n + p];
            bx[p] = x[(size_t)bj * n + p];
            by[p] = y[(size_t)bj * n + p];
            bg[p] = g;
        }
    }
    sc.ns = ns;
    sc.dev_timed = false;
    sc.launches = rounds;
    for (size_t p = 0; p < n; ++p) {
        const SizeAnswer s = size_answer(any_nan[p] != 0, max_in[p], bx[p], by[p], bg[p]);
        amount_in[p] = s.amount_in;
        amount_out[p] = s.amount_out;
        gain[p] = s.gain;
        status[p] = s.status;
    }
    return CFMM_OK;
}

void fill_args(SizeArgs& a, int64_t count, int32_t max_hops, int32_t rounds)
{
    a.p.count = count;
    a.p.max_hops = max_hops;
    a.p.hops = nullptr;
    a.rounds = rounds;
}

} // namespace

// Pinned staging behind the table (stage_layout.h SizeStage), copied to / from the scratch's device arrays in stream order; one
// synchronisation.
int cfmm_size_path(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                   const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* max_amount_in, const double* value_in,
                   const double* value_out, int32_t rounds, double* amount_in, double* amount_out, double* gain, int32_t* status)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    char msg[256] = "";
    int rc;
    if ((rc = check_size_scalars(kWho, count, max_hops, rounds, msg, sizeof msg)) ||
        (rc = check_size_arrays(kWho, count, max_amount_in, amount_in, amount_out, gain, status, msg, sizeof msg)) ||
        (rc = check_size_amounts(kWho, count, max_amount_in, value_in, value_out, msg, sizeof msg)))
        return refuse(c, rc, msg);
    const std::vector<PathSegInfo> info = seg_infos(c);
    rc = check_paths(kWho, false, info.data(), (int64_t)info.size(), count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out,
                     max_amount_in, msg, sizeof msg);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty())
        return multi_size(c, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, max_amount_in, value_in, value_out,
                          rounds, amount_in, amount_out, gain, status);

    HIP_TRY(c, hipSetDevice(c->device));
    SizeScratch& sc = c->size;
    const size_t n = (size_t)count, H = (size_t)max_hops, nh = n * H;
    const SizeStage lay = stage_of(c, n, nh);
    SizeArgs a{};
    if ((rc = sc.upload_table(c, lay, a.p.nseg)) || (rc = sc.hop_i32.grow(c, n + 3 * nh)) || (rc = sc.hop_row.grow(c, nh)) ||
        (rc = sc.in.grow(c, 3 * n)) || (rc = sc.out.grow(c, 3 * n)) || (rc = sc.status.grow(c, n)))
        return rc;
    unsigned long long* st = sc.stage.host();
    int32_t* h_i32 = lay.i32.in(st);
    long long* h_row = lay.row.in(st);
    double *h_in = lay.in.in(st), *h_out = lay.out.in(st);
    int32_t* h_status = lay.status.in(st);
    std::memcpy(h_i32, n_hops, n * sizeof(int32_t));
    std::memcpy(h_i32 + n, hop_seg, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + nh, hop_coin_in, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + 2 * nh, hop_coin_out, nh * sizeof(int32_t));
    std::memcpy(h_row, hop_row, nh * sizeof(long long));
    std::memcpy(h_in, max_amount_in, n * sizeof(double));
    for (int v = 0; v < 2; ++v) {   // (the column of a value the call does not give crosses as zeros and is never read)
        const double* value = v ? value_out : value_in;
        if (value) std::memcpy(h_in + (1 + v) * n, value, n * sizeof(double));
        else std::memset(h_in + (1 + v) * n, 0, n * sizeof(double));
    }
    HIP_TRY(c, hipMemcpyAsync(sc.hop_i32.get(), h_i32, (n + 3 * nh) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.hop_row.get(), h_row, nh * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.in.get(), h_in, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    fill_args(a, count, max_hops, rounds);
    a.p.segs = sc.table.get();
    a.p.n_hops = sc.hop_i32.get();
    a.p.hop_seg = sc.hop_i32.get() + n;
    a.p.hop_coin_in = sc.hop_i32.get() + n + nh;
    a.p.hop_coin_out = sc.hop_i32.get() + n + 2 * nh;
    a.p.hop_row = sc.hop_row.get();
    a.p.given = sc.in.get();
    a.value_in = value_in ? sc.in.get() + n : nullptr;
    a.value_out = value_out ? sc.in.get() + 2 * n : nullptr;
    a.p.answer = sc.out.get();
    a.amount_out = sc.out.get() + n;
    a.gain = sc.out.get() + 2 * n;
    a.status = sc.status.get();
    if ((rc = launch(c, a)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sc.in_flight = false;
    sc.dev_timed = false;
    if (c->opt_time_kernels != 0 && (rc = sc.ev.elapsed_ns(c, 0, 1, sc.ns)) != CFMM_OK) return rc;
    std::memcpy(amount_in, h_out, n * sizeof(double));
    std::memcpy(amount_out, h_out + n, n * sizeof(double));
    std::memcpy(gain, h_out + 2 * n, n * sizeof(double));
    std::memcpy(status, h_status, n * sizeof(int32_t));
    return CFMM_OK;
}

int cfmm_size_path_dev(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                       const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                       const double* d_max_amount_in, const double* d_value_in, const double* d_value_out, int32_t rounds,
                       double* d_amount_in, double* d_amount_out, double* d_gain, int32_t* d_status)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", kWhoDev);
    char msg[256] = "";
    int rc;
    if ((rc = check_size_scalars(kWhoDev, count, max_hops, rounds, msg, sizeof msg)) ||
        (rc = check_size_arrays(kWhoDev, count, d_max_amount_in, d_amount_in, d_amount_out, d_gain, d_status, msg, sizeof msg)))
        return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    if (!d_n_hops || !d_hop_seg || !d_hop_row || !d_hop_coin_in || !d_hop_coin_out)
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", kWhoDev);
    HIP_TRY(c, hipSetDevice(c->device));
    SizeArgs a{};
    if ((rc = c->size.upload_table(c, stage_of(c, 0, 0), a.p.nseg)) != CFMM_OK) return rc;
    fill_args(a, count, max_hops, rounds);
    a.p.segs = c->size.table.get();
    a.p.n_hops = d_n_hops;
    a.p.hop_seg = d_hop_seg;
    a.p.hop_row = reinterpret_cast<const long long*>(d_hop_row);
    a.p.hop_coin_in = d_hop_coin_in;
    a.p.hop_coin_out = d_hop_coin_out;
    a.p.given = d_max_amount_in;
    a.value_in = d_value_in;
    a.value_out = d_value_out;
    a.p.answer = d_amount_in;
    a.amount_out = d_amount_out;
    a.gain = d_gain;
    a.status = d_status;
    if ((rc = launch(c, a)) != CFMM_OK) return rc;
    c->size.dev_timed = c->opt_time_kernels != 0;   // the span is read when "size_ns" is asked for (the call does not wait)
    return CFMM_OK;
}
