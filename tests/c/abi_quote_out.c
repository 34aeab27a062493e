/* cfmm_quote_out / cfmm_quote_out_dev from plain C: a 3-pool ProductTwoCoin market, host-pointer exact-output quotes against
 * the closed form, the round trip through cfmm_quote, +inf for an output the pool cannot give (not an error), device-pointer
 * quotes (HIP runtime C API for the arrays) against the host-pointer ones, the NaN of a bad device query and the refusal of a
 * bad host query.  Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "cfmm_amd.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)
#define HIP(call)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_));                 \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    const double R[6] = {1e6, 1e6, 1e3, 2e3, 5e2, 7e2};
    const double gamma[3] = {0.997, 1.0, 0.997};
    const int32_t Ai[6] = {0, 1, 0, 1, 1, 2};
    CHECK(c, cfmm_pools_add_product(c, 3, R, gamma, Ai));

    /* five queries: a ladder of three outputs from pool 1, then pool 2, then nothing from pool 0; no sweep has run */
    const int64_t idx[5] = {1, 1, 1, 2, 0};
    const int32_t cin[5] = {0, 0, 0, 1, 1}, cout[5] = {1, 1, 1, 0, 0};
    const double want_out[5] = {1.0, 10.0, 1000.0, 35.0, 0.0};
    double in[5] = {-1, -1, -1, -1, -1}, in2[5], back[5];
    CHECK(c, cfmm_quote_out(c, 0, 5, idx, cin, cout, want_out, in));
    for (int q = 0; q < 5; ++q) {
        const double Ri = R[2 * idx[q] + cin[q]], Ro = R[2 * idx[q] + cout[q]], o = want_out[q];
        const double want = (Ri * o) / ((Ro - o) * gamma[idx[q]]);
        printf("quote_out %d: pool %lld coin %d wanted %.17g -> %.17g\n", q, (long long)idx[q], cin[q], o, in[q]);
        if (in[q] != want) return 3;
    }
    if (!(in[0] < in[1] && in[1] < in[2] && in[2] / 1000.0 > in[0]) || in[4] != 0.0 || signbit(in[4])) return 4;
    CHECK(c, cfmm_quote_out(c, 0, 5, idx, cin, NULL, want_out, in2));      /* coin_out == NULL: the other coin */
    if (memcmp(in, in2, sizeof in)) return 5;
    CHECK(c, cfmm_quote_out(c, 0, 0, NULL, NULL, NULL, NULL, NULL));       /* count == 0: a no-op */
    CHECK(c, cfmm_quote(c, 0, 5, idx, cin, cout, in, back));               /* tendering the answer yields the wanted output */
    for (int q = 0; q < 5; ++q)
        if (fabs(back[q] - want_out[q]) > 1e-12 * want_out[q]) return 12;

    /* more than the pool holds is not an error: +inf for that query */
    const double too_much[5] = {1.0, 2e3, 3e3, 35.0, 0.0};                 /* pool 1 holds 2e3 of coin 1 */
    CHECK(c, cfmm_quote_out(c, 0, 5, idx, cin, cout, too_much, in2));
    printf("beyond the reserve: %.17g %.17g\n", in2[1], in2[2]);
    if (in2[0] != in[0] || !isinf(in2[1]) || !isinf(in2[2]) || in2[1] < 0 || in2[3] != in[3]) return 13;

    /* refused before anything runs: the query is named, the outputs stay */
    const double bad_amt[5] = {1.0, -1.0, 100.0, 35.0, 0.0};
    double keep[5] = {7, 7, 7, 7, 7};
    if (cfmm_quote_out(c, 0, 5, idx, cin, cout, bad_amt, keep) != CFMM_ERR_INVALID_ARG) return 6;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "query 1") || strncmp(cfmm_last_error(c), "cfmm_quote_out:", 15)) return 7;
    for (int q = 0; q < 5; ++q)
        if (keep[q] != 7) return 8;
    if (cfmm_quote_out(c, 1, 1, idx, cin, cout, want_out, keep) != CFMM_ERR_INVALID_ARG) return 9;

    /* device pointers: the same five queries, then one with a row out of range -> NaN for that query alone */
    int64_t* d_idx; int32_t *d_cin, *d_cout; double *d_amt, *d_out;
    HIP(hipMalloc((void**)&d_idx, sizeof idx));
    HIP(hipMalloc((void**)&d_cin, sizeof cin));
    HIP(hipMalloc((void**)&d_cout, sizeof cout));
    HIP(hipMalloc((void**)&d_amt, sizeof want_out));
    HIP(hipMalloc((void**)&d_out, sizeof in));
    int64_t idx_bad[5];
    memcpy(idx_bad, idx, sizeof idx);
    idx_bad[3] = 3;                                                    /* the segment has rows 0..2 */
    HIP(hipMemcpy(d_idx, idx_bad, sizeof idx, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_cin, cin, sizeof cin, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_cout, cout, sizeof cout, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_amt, want_out, sizeof want_out, hipMemcpyHostToDevice));
    CHECK(c, cfmm_quote_out_dev(c, 0, 5, d_idx, d_cin, d_cout, d_amt, d_out));
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(in2, d_out, sizeof in, hipMemcpyDeviceToHost));
    for (int q = 0; q < 5; ++q) {
        printf("quote_out_dev %d -> %.17g\n", q, in2[q]);
        if (q == 3 ? !isnan(in2[q]) : in2[q] != in[q]) return 10;
    }
    if (cfmm_quote_out_dev(c, 0, -1, d_idx, d_cin, d_cout, d_amt, d_out) != CFMM_ERR_INVALID_ARG) return 11;
    HIP(hipFree(d_idx)); HIP(hipFree(d_cin)); HIP(hipFree(d_cout)); HIP(hipFree(d_amt)); HIP(hipFree(d_out));
    cfmm_ctx_destroy(c);
    printf("abi_quote_out: ok\n");
    return 0;
}
