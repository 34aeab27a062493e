/* cfmm_swap from plain C: a market with one segment of every kind.  One swap per kind -- the answer is cfmm_quote's, the pool
 * has moved (Product: to exactly R + gamma*a and R - out) --, a row repeated in one call against the same swaps one call
 * each, a swap that would empty a pool (NaN, the pool stays, "swap_refused"), a refused call (the query named, outputs and
 * pools untouched) and the state protocol (earlier trades are gone).  Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

static int upload(cfmm_ctx* c)
{
    const double R2[6] = {1e6, 1e6, 1e3, 2e3, 5e2, 7e2}, g3[3] = {0.997, 1.0, 0.997}, w2[6] = {0.3, 0.7, 0.5, 0.5, 0.8, 0.2};
    const int32_t Ai2[6] = {0, 1, 0, 1, 1, 2};
    CHECK(c, cfmm_pools_add_product(c, 3, R2, g3, Ai2));                                   /* segment 0 */
    CHECK(c, cfmm_pools_add_geomean(c, 3, R2, w2, g3, Ai2));                               /* segment 1 */
    const double cp[2] = {0.6, 2.25}, gu[2] = {0.997, 1.0}, lt[6] = {4.0, 1.0, 0.25, 4.0, 1.0, 0.25};
    const double lq[6] = {16.0, 16.0, 16.0, 144.0, 144.0, 144.0};
    const int64_t off[3] = {0, 3, 6};
    const int32_t Aiu[4] = {0, 1, 1, 2};
    CHECK(c, cfmm_pools_add_univ3(c, 2, cp, gu, Aiu, off, lt, lq));                        /* segment 2 */
    const double R3[6] = {1e3, 2e3, 3e3, 4e3, 5e3, 6e3}, w3[6] = {0.2, 0.3, 0.5, 1.0, 1.0, 2.0}, gg[2] = {0.997, 0.9995};
    const int32_t Ai3[6] = {0, 1, 2, 2, 1, 0};
    CHECK(c, cfmm_pools_add_weighted(c, 2, 3, R3, w3, gg, Ai3));                           /* segment 3 */
    const double Rc[6] = {1e4, 1.1e4, 0.9e4, 2e4, 2.1e4, 1.9e4}, al[2] = {2.0, 50.0}, be[2] = {1e16, 1.6e17};
    CHECK(c, cfmm_pools_add_curve(c, 2, 3, Rc, gg, Ai3, al, be));                          /* segment 4 */
    CHECK(c, cfmm_pools_add_solidly(c, 3, R2, g3, Ai2));                                   /* segment 5 */
    return 0;
}

int main(void)
{
    cfmm_ctx *c = NULL, *t = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK || cfmm_ctx_create(0, 3, &t) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    if (upload(c) || upload(t)) return 2;
    const double v[3] = {1.0, 1.3, 0.8};
    double D[64], L[64];
    CHECK(c, cfmm_find_arb(c, v));
    CHECK(c, cfmm_get_trades(c, D, L));

    /* one swap per kind: pool 1 of each segment, coin 0 for coin 1; the answer is the quote's, the next quote is smaller */
    const int64_t row1 = 1;
    const int32_t c0 = 0, c1 = 1;
    for (int seg = 0; seg < 6; ++seg) {
        const double amt = seg == 2 ? 4.0 : 25.0;
        double q = -1, s = -1, after = -1;
        CHECK(c, cfmm_quote(c, seg, 1, &row1, &c0, &c1, &amt, &q));
        CHECK(c, cfmm_swap(c, seg, 1, &row1, &c0, &c1, &amt, &s));
        CHECK(c, cfmm_quote(c, seg, 1, &row1, &c0, &c1, &amt, &after));
        printf("swap seg %d: quote %.17g swap %.17g next quote %.17g\n", seg, q, s, after);
        if (memcmp(&q, &s, sizeof q) || !(s > 0) || !(after < s)) return 3;
    }
    /* ... the earlier trades described the old market */
    if (cfmm_get_trades(c, D, L) != CFMM_ERR_STATE || !strstr(cfmm_last_error(c), "no materialised trades")) return 4;
    double R[6], P[2];
    CHECK(c, cfmm_get_reserves(c, 0, R));
    {
        const double x = 1.0 * 25.0, out = 2e3 * (x / (1e3 + x));
        if (R[2] != 1e3 + x || R[3] != 2e3 - out || R[0] != 1e6 || R[5] != 7e2) return 5;
    }
    CHECK(c, cfmm_get_prices(c, 2, P));
    printf("univ3 prices after the swap: %.17g %.17g\n", P[0], P[1]);
    if (P[0] != 0.6 || P[1] != 1.0) return 6;      /* 4 of coin 0 from 2.25 ends exactly on the tick edge at 1 */

    /* a row repeated in one call (on the untouched twin) == the same swaps one call each */
    const int64_t rows[4] = {2, 0, 2, 2};
    const int32_t cin[4] = {0, 1, 1, 0};
    const double amt[4] = {10.0, 50.0, 20.0, 5.0};
    double batch[4], single[4], Rb[6], Rs[6];
    CHECK(t, cfmm_swap(t, 0, 4, rows, cin, NULL, amt, batch));
    CHECK(t, cfmm_get_reserves(t, 0, Rb));
    CHECK(c, cfmm_pools_clear(c));
    if (upload(c)) return 2;
    for (int q = 0; q < 4; ++q) CHECK(c, cfmm_swap(c, 0, 1, rows + q, cin + q, NULL, amt + q, single + q));
    CHECK(c, cfmm_get_reserves(c, 0, Rs));
    for (int q = 0; q < 4; ++q) printf("repeated row: query %d batch %.17g single %.17g\n", q, batch[q], single[q]);
    if (memcmp(batch, single, sizeof batch) || memcmp(Rb, Rs, sizeof Rb)) return 7;

    /* a swap that would empty the pool: NaN, the pool stays, the call succeeds; the next swap of the row proceeds */
    const int64_t r2[2] = {1, 1};
    const int32_t i2[2] = {0, 0};
    const double a2[2] = {1e40, 1.0};
    double o2[2];
    int64_t refused = -1;
    CHECK(c, cfmm_get_reserves(c, 0, Rs));
    CHECK(c, cfmm_swap(c, 0, 2, r2, i2, NULL, a2, o2));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    CHECK(c, cfmm_get_reserves(c, 0, R));
    printf("refused swap: %.17g then %.17g, swap_refused %lld\n", o2[0], o2[1], (long long)refused);
    if (!isnan(o2[0]) || refused != 1 || o2[1] != Rs[3] * (1.0 / (Rs[2] + 1.0))) return 8;
    if (R[2] != Rs[2] + 1.0 || R[3] != Rs[3] - o2[1]) return 9;

    /* a refused call: the query is named, outputs and pools are untouched */
    const double bad[4] = {10.0, 50.0, -1.0, 5.0};
    double keep[4] = {7, 7, 7, 7};
    if (cfmm_swap(c, 0, 4, rows, cin, NULL, bad, keep) != CFMM_ERR_INVALID_ARG) return 10;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strncmp(cfmm_last_error(c), "cfmm_swap:", 10) || !strstr(cfmm_last_error(c), "query 2")) return 11;
    for (int q = 0; q < 4; ++q)
        if (keep[q] != 7) return 12;
    CHECK(c, cfmm_get_reserves(c, 0, Rs));
    if (memcmp(R, Rs, sizeof R)) return 13;
    if (cfmm_swap(c, 3, 1, &row1, &c0, NULL, amt, keep) != CFMM_ERR_INVALID_ARG || !strstr(cfmm_last_error(c), "coin_out is required")) return 14;
    if (cfmm_swap(c, 6, 1, &row1, &c0, &c1, amt, keep) != CFMM_ERR_INVALID_ARG) return 15;
    CHECK(c, cfmm_swap(c, 0, 0, NULL, NULL, NULL, NULL, NULL));       /* count == 0: a no-op */
    cfmm_ctx_destroy(c);
    cfmm_ctx_destroy(t);
    printf("abi_swap: ok\n");
    return 0;
}
