// Host build of csrc/univ3_pool.h for tests/test_pool_update_cpu.py: m UniV3 pools prepared ONE BY ONE with
// univ3_prepare_pool (the function both the upload and cfmm_pools_set_prices call), thresholds and heads as the upload
// forms them, into flat arrays in the layout of tests/golden/univ3_prepare_parent.npz.  Returns the number of records.
#include "univ3_pool.h"

using namespace cfmm;

extern "C" long long univ3_prepare_host(long long m, const double* cp, const double* gamma, const int64_t* off, const double* lt,
                                        const double* lq, double* pg, double* cur_a, double* cur_b, double* cur_c, double* curR,
                                        int32_t* walk, double* ticks_out, double* thr_out, uint32_t* head)
{
    std::vector<TickRec> ticks;
    std::vector<int4> w((size_t)m);
    for (long long i = 0; i < m; ++i) {
        const int64_t o = off[i], nt = off[i + 1] - o;
        const int64_t ct = univ3_current_tick(lt + o, nt, cp[i]);
        if (ct < 1) return -1 - i;
        UniV3PoolRec r;
        univ3_prepare_pool(cp[i], gamma[i], ct, nt, lt + o, lq + o, r, ticks);
        reinterpret_cast<double2*>(pg)[i] = r.pg;
        reinterpret_cast<double2*>(cur_a)[i] = r.cur_a;
        reinterpret_cast<double2*>(cur_b)[i] = r.cur_b;
        reinterpret_cast<double2*>(curR)[i] = r.curR;
        cur_c[i] = r.cur_c;
        w[(size_t)i] = r.walk;
        std::memcpy(walk + 4 * i, &r.walk, sizeof r.walk);
    }
    std::vector<double> thr;
    univ3_all_thresholds(ticks, thr);
    thr.resize(ticks.size() + 4, 0.0);
    for (long long i = 0; i < m; ++i) univ3_heads(w[(size_t)i], thr.data(), reinterpret_cast<uint4*>(head) + 2 * i);
    std::memcpy(ticks_out, ticks.data(), ticks.size() * sizeof(TickRec));
    std::memcpy(thr_out, thr.data(), thr.size() * sizeof(double));
    return (long long)ticks.size();
}
