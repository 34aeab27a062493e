/* cfmm_quote / cfmm_quote_dev from plain C: a 3-pool ProductTwoCoin market, host-pointer quotes against the closed form,
 * device-pointer quotes (HIP runtime C API for the arrays) against the host-pointer ones, the NaN of a bad device query and
 * the refusal of a bad host query.  Exit code 0 = everything held. */
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

    /* five queries: a ladder of three sizes through pool 1, then pools 2 and 0; no sweep has run */
    const int64_t idx[5] = {1, 1, 1, 2, 0};
    const int32_t cin[5] = {0, 0, 0, 1, 1}, cout[5] = {1, 1, 1, 0, 0};
    const double amt[5] = {1.0, 10.0, 100.0, 35.0, 0.0};
    double out[5] = {-1, -1, -1, -1, -1}, out2[5];
    CHECK(c, cfmm_quote(c, 0, 5, idx, cin, cout, amt, out));
    for (int q = 0; q < 5; ++q) {
        const double Ri = R[2 * idx[q] + cin[q]], Ro = R[2 * idx[q] + cout[q]], x = gamma[idx[q]] * amt[q];
        const double want = Ro * (x / (Ri + x));
        printf("quote %d: pool %lld coin %d amount %.17g -> %.17g\n", q, (long long)idx[q], cin[q], amt[q], out[q]);
        if (out[q] != want) return 3;
    }
    if (!(out[0] < out[1] && out[1] < out[2] && out[2] / 100.0 < out[0]) || out[4] != 0.0 || signbit(out[4])) return 4;
    CHECK(c, cfmm_quote(c, 0, 5, idx, cin, NULL, amt, out2));          /* coin_out == NULL: the other coin */
    if (memcmp(out, out2, sizeof out)) return 5;
    CHECK(c, cfmm_quote(c, 0, 0, NULL, NULL, NULL, NULL, NULL));       /* count == 0: a no-op */

    /* refused before anything runs: the query is named, the outputs stay */
    const double bad_amt[5] = {1.0, -1.0, 100.0, 35.0, 0.0};
    double keep[5] = {7, 7, 7, 7, 7};
    if (cfmm_quote(c, 0, 5, idx, cin, cout, bad_amt, keep) != CFMM_ERR_INVALID_ARG) return 6;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "query 1")) return 7;
    for (int q = 0; q < 5; ++q)
        if (keep[q] != 7) return 8;
    if (cfmm_quote(c, 1, 1, idx, cin, cout, amt, keep) != CFMM_ERR_INVALID_ARG) return 9;

    /* device pointers: the same five queries, then one with a row out of range -> NaN for that query alone */
    int64_t* d_idx; int32_t *d_cin, *d_cout; double *d_amt, *d_out;
    HIP(hipMalloc((void**)&d_idx, sizeof idx));
    HIP(hipMalloc((void**)&d_cin, sizeof cin));
    HIP(hipMalloc((void**)&d_cout, sizeof cout));
    HIP(hipMalloc((void**)&d_amt, sizeof amt));
    HIP(hipMalloc((void**)&d_out, sizeof out));
    int64_t idx_bad[5];
    memcpy(idx_bad, idx, sizeof idx);
    idx_bad[3] = 3;                                                    /* the segment has rows 0..2 */
    HIP(hipMemcpy(d_idx, idx_bad, sizeof idx, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_cin, cin, sizeof cin, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_cout, cout, sizeof cout, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_amt, amt, sizeof amt, hipMemcpyHostToDevice));
    CHECK(c, cfmm_quote_dev(c, 0, 5, d_idx, d_cin, d_cout, d_amt, d_out));
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(out2, d_out, sizeof out, hipMemcpyDeviceToHost));
    for (int q = 0; q < 5; ++q) {
        printf("quote_dev %d -> %.17g\n", q, out2[q]);
        if (q == 3 ? !isnan(out2[q]) : out2[q] != out[q]) return 10;
    }
    if (cfmm_quote_dev(c, 0, -1, d_idx, d_cin, d_cout, d_amt, d_out) != CFMM_ERR_INVALID_ARG) return 11;
    HIP(hipFree(d_idx)); HIP(hipFree(d_cin)); HIP(hipFree(d_cout)); HIP(hipFree(d_amt)); HIP(hipFree(d_out));
    cfmm_ctx_destroy(c);
    printf("abi_quote: ok\n");
    return 0;
}
