/* cfmm_size_path from plain C: three ProductTwoCoin pools that quote slightly different prices for three tokens, the cycle
 * 0 -> 1 -> 2 -> 0 through them sized with two limits (one far above the optimum, one that binds), the round trip through
 * cfmm_quote_path bit for bit, the gain as "out minus in", a cycle that gains nothing, and one refused call that names the path.
 * Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_size_path.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

enum { P = 3, H = 3 };   /* paths, max_hops */

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    /* 0 -> 1 at about 2.00, 1 -> 2 at about 0.52, 2 -> 0 at about 1.00: 1.04 round the cycle before fees */
    const double R[6] = {1.00e5, 2.00e5, 2.00e5, 1.04e5, 1.0e5, 1.0e5};
    const double gamma[3] = {0.997, 0.997, 0.9995};
    const int32_t Ai[6] = {0, 1, 1, 2, 2, 0};
    CHECK(c, cfmm_pools_add_product(c, 3, R, gamma, Ai));

    /* hop-major: entry k*P + p.  Paths 0 and 1: the cycle.  Path 2: the cycle backwards, which loses at every size. */
    const int32_t n_hops[P] = {3, 3, 3};
    const int32_t seg[H * P] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t row[H * P] = {0, 0, 2, /**/ 1, 1, 1, /**/ 2, 2, 0};
    const int32_t cin[H * P] = {0, 0, 1, /**/ 0, 0, 1, /**/ 0, 0, 1};
    const int32_t cout[H * P] = {1, 1, 0, /**/ 1, 1, 0, /**/ 1, 1, 0};
    const double max_in[P] = {5000.0, 10.0, 5000.0};
    double x[P], y[P], g[P], back[P];
    int32_t st[P];
    CHECK(c, cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, max_in, NULL, NULL, 5, x, y, g, st));
    for (int p = 0; p < P; ++p) printf("path %d: status %d, %.17g in -> %.17g out, gain %.17g\n", p, (int)st[p], x[p], y[p], g[p]);
    if (st[0] != CFMM_SIZED || !(x[0] > 0 && x[0] < max_in[0]) || !(g[0] > 0)) return 3;
    if (st[1] != CFMM_SIZED_AT_LIMIT || memcmp(&x[1], &max_in[1], sizeof(double)) || !(g[1] > 0 && g[1] < g[0])) return 4;
    if (st[2] != CFMM_SIZED_NONE || x[2] != 0.0 || y[2] != 0.0 || g[2] != 0.0 || signbit(x[2]) || signbit(y[2]) || signbit(g[2])) return 5;
    /* the round trip: cfmm_quote_path at the returned amount_in answers amount_out bit for bit; the gain is out minus in */
    CHECK(c, cfmm_quote_path(c, P, H, n_hops, seg, row, cin, cout, x, back, NULL));
    if (memcmp(back, y, sizeof y)) return 6;
    for (int p = 0; p < 2; ++p) {
        const double d = y[p] - x[p];
        if (memcmp(&d, &g[p], sizeof d)) return 7;
    }
    /* more rounds do not lose: the gain of 8 rounds is within a hair of that of 5, and one round is a coarser answer */
    double x1[P], y1[P], g1[P], g8[P];
    int32_t st1[P];
    CHECK(c, cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, max_in, NULL, NULL, 1, x1, y1, g1, st1));
    CHECK(c, cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, max_in, NULL, NULL, 8, x1, y1, g8, st1));
    if (!(g1[0] > 0 && g1[0] <= g[0]) || fabs(g8[0] - g[0]) > 1e-9 * g[0]) return 8;
    /* valued at twice the output, the input is never worth tendering */
    const double two[P] = {2.0, 2.0, 2.0};
    CHECK(c, cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, max_in, two, NULL, 5, x1, y1, g1, st1));
    if (st1[0] != CFMM_SIZED_NONE || st1[1] != CFMM_SIZED_NONE) return 9;
    CHECK(c, cfmm_size_path(c, 0, H, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */

    /* refused before anything runs: the path is named, the outputs stay */
    double keep[P] = {7, 7, 7};
    int32_t keep_st[P] = {7, 7, 7};
    const double bad_in[P] = {5000.0, -1.0, 5000.0};
    if (cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, bad_in, NULL, NULL, 5, keep, keep, keep, keep_st) != CFMM_ERR_INVALID_ARG) return 10;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "path 1, hop 0: max_amount_in") || strncmp(cfmm_last_error(c), "cfmm_size_path:", 15)) return 11;
    if (cfmm_size_path(c, P, H, n_hops, seg, row, cin, cout, max_in, NULL, NULL, CFMM_MAX_SIZE_ROUNDS + 1, keep, keep, keep, keep_st) != CFMM_ERR_INVALID_ARG) return 12;
    if (!strstr(cfmm_last_error(c), "rounds must be 1 .. 16")) return 13;
    for (int i = 0; i < P; ++i)
        if (keep[i] != 7 || keep_st[i] != 7) return 14;
    if (cfmm_size_path_dev(c, -1, H, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL) != CFMM_ERR_INVALID_ARG) return 15;
    cfmm_ctx_destroy(c);
    printf("abi_size_path: ok\n");
    return 0;
}
