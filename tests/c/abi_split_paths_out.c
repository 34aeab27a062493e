/* cfmm_split_paths_out from plain C: abi_split_paths.c's market (three ProductTwoCoin pools 0 -> 1 of different depth, the
 * two-hop detour 0 -> 2 -> 1 and a deep pool).  Order 0 wants 150 000 of token 1 over the four paths -- more than any single
 * path can give, so cfmm_quote_path_out answers +inf for each, and the split fills it; order 1 buys through the deep pool alone;
 * order 2 wants nothing; order 3 wants more than its two paths hold.  The shares sum to the amount, the round trip through
 * cfmm_quote_path_out holds bit for bit, the one-path order gets its amount bit for bit, and two refused calls name the order.
 * Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_split_out.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

enum { G = 4, P = 8, H = 2 };   /* orders, paths, max_hops */

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    const double R[12] = {1.0e5, 1.0e5, 5.0e4, 5.0e4, 2.0e4, 2.0e4, 8.0e4, 8.0e4, 8.0e4, 8.0e4, 1.0e6, 1.0e6};
    const double gamma[6] = {0.997, 0.997, 0.999, 0.997, 0.997, 0.997};
    const int32_t Ai[12] = {0, 1, 0, 1, 0, 1, 0, 2, 2, 1, 0, 1};
    CHECK(c, cfmm_pools_add_product(c, 6, R, gamma, Ai));

    /* hop-major: entry k*P + p.  Order 0: paths 0 .. 3 (three pools and the detour); order 1: path 4 (the deep pool alone);
     * order 2: path 5 (pool 0 again -- another order may use it) with nothing to buy; order 3: paths 6 and 7 (pools 1 and 2) */
    const int64_t first[G + 1] = {0, 4, 5, 6, 8};
    const double amount[G] = {1.5e5, 12345.678, 0.0, 1.0e5};
    const int32_t n_hops[P] = {1, 1, 1, 2, 1, 1, 1, 1};
    const int32_t seg[H * P] = {0};
    const int64_t row[H * P] = {0, 1, 2, 3, 5, 0, 1, 2, /**/ 0, 0, 0, 4, 0, 0, 0, 0};
    const int32_t cin[H * P] = {0};
    const int32_t cout[H * P] = {1, 1, 1, 1, 1, 1, 1, 1, /**/ 1, 1, 1, 1, 1, 1, 1, 1};
    double x[P], cost[P], total[G], back[P], alone[P];
    int32_t st[G];
    CHECK(c, cfmm_split_paths_out(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 5, x, cost, total, st));
    for (int p = 0; p < P; ++p) printf("path %d: buys %.17g for %.17g\n", p, x[p], cost[p]);
    for (int g = 0; g < G; ++g) printf("order %d: status %d, total %.17g\n", g, (int)st[g], total[g]);
    if (st[0] != CFMM_SPLIT_OK || st[1] != CFMM_SPLIT_OK || st[2] != CFMM_SPLIT_NONE || st[3] != CFMM_SPLIT_UNOBTAINABLE) return 3;
    const double sum = x[0] + x[1] + x[2] + x[3];
    if (fabs(sum - amount[0]) > 1e-15 * amount[0] || !(x[0] > x[1] && x[1] > x[2] && x[2] > 0 && x[3] > 0)) return 4;   /* deeper pools give more */
    if (!(x[0] < 1.0e5 && x[1] < 5.0e4 && x[2] < 2.0e4 && x[3] < 8.0e4) || !isfinite(total[0])) return 4;               /* each below its pool's reserve */
    if (memcmp(&x[4], &amount[1], sizeof(double))) return 5;                       /* one path: the amount, bit for bit */
    if (x[5] != 0.0 || cost[5] != 0.0 || total[2] != 0.0 || signbit(x[5]) || signbit(cost[5]) || signbit(total[2])) return 6;
    if (!(isinf(total[3]) && total[3] > 0 && isinf(cost[6]) && isinf(cost[7])) || x[6] != 0.0 || x[7] != 0.0 || signbit(x[6])) return 6;
    /* the round trip, and the total as the sum in path order */
    CHECK(c, cfmm_quote_path_out(c, P, H, n_hops, seg, row, cin, cout, x, back, NULL));
    if (memcmp(back, cost, 5 * sizeof(double))) return 7;
    const double t0 = ((cost[0] + cost[1]) + cost[2]) + cost[3];
    if (memcmp(&t0, &total[0], sizeof t0) || memcmp(&cost[4], &total[1], sizeof(double))) return 8;
    /* the whole amount through any single path of order 0 cannot be had */
    const double all[P] = {amount[0], amount[0], amount[0], amount[0], amount[1], 0.0, 0.0, 0.0};
    CHECK(c, cfmm_quote_path_out(c, P, H, n_hops, seg, row, cin, cout, all, alone, NULL));
    for (int p = 0; p < 4; ++p)
        if (!(isinf(alone[p]) && alone[p] > 0)) return 9;
    printf("split %.9g where every single path answers inf\n", total[0]);
    /* one round is a coarser answer, eight rounds do not lose */
    double x1[P], c1[P], t1[G], t8[G];
    int32_t st1[G];
    CHECK(c, cfmm_split_paths_out(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 1, x1, c1, t1, st1));
    CHECK(c, cfmm_split_paths_out(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 8, x1, c1, t8, st1));
    if (!(t1[0] >= total[0]) || fabs(t8[0] - total[0]) > 1e-6 * total[0]) return 10;
    CHECK(c, cfmm_split_paths_out(c, 0, NULL, NULL, 0, H, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */

    /* refused before anything runs: the order is named, the outputs stay */
    double keep[P] = {7, 7, 7, 7, 7, 7, 7, 7}, keep_t[G] = {7, 7, 7, 7};
    int32_t keep_st[G] = {7, 7, 7, 7};
    const int64_t shared_row[H * P] = {0, 1, 0, 3, 5, 0, 1, 2, /**/ 0, 0, 0, 4, 0, 0, 0, 0};   /* order 0: paths 0 and 2 through pool 0 */
    if (cfmm_split_paths_out(c, G, first, amount, P, H, n_hops, seg, shared_row, cin, cout, 5, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 11;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strcmp(cfmm_last_error(c), "cfmm_split_paths_out: order 0: paths 0 and 2 share pool (segment 0, row 0)")) return 12;
    const double bad_amount[G] = {1.0e5, -1.0, 0.0, 1.0};
    if (cfmm_split_paths_out(c, G, first, bad_amount, P, H, n_hops, seg, row, cin, cout, 5, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 13;
    if (!strstr(cfmm_last_error(c), "order 1: amount_out must be finite and >= 0")) return 14;
    if (cfmm_split_paths_out(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, CFMM_MAX_SPLIT_ROUNDS + 1, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 15;
    if (!strstr(cfmm_last_error(c), "rounds must be 1 .. 16")) return 16;
    for (int i = 0; i < P; ++i)
        if (keep[i] != 7) return 17;
    for (int i = 0; i < G; ++i)
        if (keep_t[i] != 7 || keep_st[i] != 7) return 17;
    if (cfmm_split_paths_out_dev(c, -1, NULL, NULL, 0, H, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL) != CFMM_ERR_INVALID_ARG) return 18;
    cfmm_ctx_destroy(c);
    printf("abi_split_paths_out: ok\n");
    return 0;
}
