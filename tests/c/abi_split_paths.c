/* cfmm_split_paths from plain C: three ProductTwoCoin pools 0 -> 1 of different depth and a two-hop detour 0 -> 2 -> 1, one order
 * over the four paths and one over the single deepest pool; the shares sum to the amount, the split beats every single path,
 * the round trip through cfmm_quote_path holds bit for bit, the one-path order gets its amount bit for bit, an empty order
 * answers zeros, and two refused calls name the order.  Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_split.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

enum { G = 3, P = 6, H = 2 };   /* orders, paths, max_hops */

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    /* pools 0 .. 2 trade token 0 for token 1 at about 1.00; pools 3 and 4 are the detour 0 -> 2 -> 1; pool 5 is deep */
    const double R[12] = {1.0e5, 1.0e5, 5.0e4, 5.0e4, 2.0e4, 2.0e4, 8.0e4, 8.0e4, 8.0e4, 8.0e4, 1.0e6, 1.0e6};
    const double gamma[6] = {0.997, 0.997, 0.999, 0.997, 0.997, 0.997};
    const int32_t Ai[12] = {0, 1, 0, 1, 0, 1, 0, 2, 2, 1, 0, 1};
    CHECK(c, cfmm_pools_add_product(c, 6, R, gamma, Ai));

    /* hop-major: entry k*P + p.  Order 0: paths 0 .. 3 (three pools and the detour); order 1: path 4 (the deep pool alone);
     * order 2: path 5 (pool 0 again -- another order may use it) with nothing to spread */
    const int64_t first[G + 1] = {0, 4, 5, 6};
    const double amount[G] = {1.0e5, 12345.678, 0.0};
    const int32_t n_hops[P] = {1, 1, 1, 2, 1, 1};
    const int32_t seg[H * P] = {0, 0, 0, 0, 0, 0, /**/ 0, 0, 0, 0, 0, 0};
    const int64_t row[H * P] = {0, 1, 2, 3, 5, 0, /**/ 0, 0, 0, 4, 0, 0};
    const int32_t cin[H * P] = {0, 0, 0, 0, 0, 0, /**/ 0, 0, 0, 0, 0, 0};
    const int32_t cout[H * P] = {1, 1, 1, 1, 1, 1, /**/ 1, 1, 1, 1, 1, 1};
    double x[P], y[P], total[G], back[P], alone[P];
    int32_t st[G];
    CHECK(c, cfmm_split_paths(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 5, x, y, total, st));
    for (int p = 0; p < P; ++p) printf("path %d: %.17g in -> %.17g out\n", p, x[p], y[p]);
    for (int g = 0; g < G; ++g) printf("order %d: status %d, total %.17g\n", g, (int)st[g], total[g]);
    if (st[0] != CFMM_SPLIT_OK || st[1] != CFMM_SPLIT_OK || st[2] != CFMM_SPLIT_NONE) return 3;
    const double sum = x[0] + x[1] + x[2] + x[3];
    if (fabs(sum - amount[0]) > 1e-15 * amount[0] || !(x[0] > x[1] && x[1] > x[2] && x[2] > 0 && x[3] > 0)) return 4;   /* deeper pools take more */
    if (memcmp(&x[4], &amount[1], sizeof(double))) return 5;                       /* one path: the amount, bit for bit */
    if (x[5] != 0.0 || y[5] != 0.0 || total[2] != 0.0 || signbit(x[5]) || signbit(y[5]) || signbit(total[2])) return 6;
    /* the round trip, and the total as the sum in path order */
    CHECK(c, cfmm_quote_path(c, P, H, n_hops, seg, row, cin, cout, x, back, NULL));
    if (memcmp(back, y, 5 * sizeof(double))) return 7;
    const double t0 = ((y[0] + y[1]) + y[2]) + y[3];
    if (memcmp(&t0, &total[0], sizeof t0) || memcmp(&y[4], &total[1], sizeof(double))) return 8;
    /* the whole amount through any single path gives less */
    const double all[P] = {amount[0], amount[0], amount[0], amount[0], amount[1], 0.0};
    CHECK(c, cfmm_quote_path(c, P, H, n_hops, seg, row, cin, cout, all, alone, NULL));
    for (int p = 0; p < 4; ++p)
        if (!(alone[p] < total[0])) return 9;
    printf("split %.9g against the best single path %.9g\n", total[0], alone[0]);
    /* one round is a coarser answer, eight rounds do not lose */
    double x1[P], y1[P], t1[G], t8[G];
    int32_t st1[G];
    CHECK(c, cfmm_split_paths(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 1, x1, y1, t1, st1));
    CHECK(c, cfmm_split_paths(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, 8, x1, y1, t8, st1));
    if (!(t1[0] > alone[0] && t1[0] <= total[0]) || fabs(t8[0] - total[0]) > 1e-6 * total[0]) return 10;
    CHECK(c, cfmm_split_paths(c, 0, NULL, NULL, 0, H, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */

    /* refused before anything runs: the order is named, the outputs stay */
    double keep[P] = {7, 7, 7, 7, 7, 7}, keep_t[G] = {7, 7, 7};
    int32_t keep_st[G] = {7, 7, 7};
    const int64_t shared_row[H * P] = {0, 1, 0, 3, 5, 0, /**/ 0, 0, 0, 4, 0, 0};   /* order 0: paths 0 and 2 through pool 0 */
    if (cfmm_split_paths(c, G, first, amount, P, H, n_hops, seg, shared_row, cin, cout, 5, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 11;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strcmp(cfmm_last_error(c), "cfmm_split_paths: order 0: paths 0 and 2 share pool (segment 0, row 0)")) return 12;
    const double bad_amount[G] = {1.0e5, -1.0, 0.0};
    if (cfmm_split_paths(c, G, first, bad_amount, P, H, n_hops, seg, row, cin, cout, 5, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 13;
    if (!strstr(cfmm_last_error(c), "order 1: amount_in must be finite and >= 0")) return 14;
    if (cfmm_split_paths(c, G, first, amount, P, H, n_hops, seg, row, cin, cout, CFMM_MAX_SPLIT_ROUNDS + 1, keep, keep, keep_t, keep_st) != CFMM_ERR_INVALID_ARG) return 15;
    if (!strstr(cfmm_last_error(c), "rounds must be 1 .. 16")) return 16;
    for (int i = 0; i < P; ++i)
        if (keep[i] != 7) return 17;
    for (int i = 0; i < G; ++i)
        if (keep_t[i] != 7 || keep_st[i] != 7) return 17;
    if (cfmm_split_paths_dev(c, -1, NULL, NULL, 0, H, NULL, NULL, NULL, NULL, NULL, 5, NULL, NULL, NULL, NULL) != CFMM_ERR_INVALID_ARG) return 18;
    cfmm_ctx_destroy(c);
    printf("abi_split_paths: ok\n");
    return 0;
}
