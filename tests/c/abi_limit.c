/* cfmm_quote_to_rate / cfmm_swap_limit from plain C: a market with one pool of each of the six kinds.  Per kind: the amount
 * to a limit of 0.9 of the spot rate, the rate cfmm_quote_rate reports at that amount (the limit again), the amount out against
 * cfmm_quote bit for bit, exactly +0.0 for a limit above the spot rate; then a limited swap of "as much as it takes", after
 * which the spot rate is the limit and a second swap finds nothing to do; and the refusals with their messages and untouched
 * outputs.  Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_limit.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
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
    const double R2[2] = {1e6, 2e6}, w2[2] = {0.3, 0.7}, gamma[1] = {0.997};
    const int32_t A01[2] = {0, 1}, A12[2] = {1, 2}, A012[3] = {0, 1, 2};
    const double R3[3] = {1e6, 1.1e6, 0.9e6}, w3[3] = {0.2, 0.3, 0.5}, alpha[1] = {2.0}, beta[1] = {1e23};
    const double price[1] = {1.0}, lower[3] = {1.2, 0.9, 0.7}, liq[3] = {1e12, 2e12, 1e12};
    const int64_t off[2] = {0, 3};
    /* segments 0..5: Product, GeometricMean, UniV3, weighted (3 coins), Curve (3 coins), Solidly */
    CHECK(c, cfmm_pools_add_product(c, 1, R2, gamma, A01));
    CHECK(c, cfmm_pools_add_geomean(c, 1, R2, w2, gamma, A01));
    CHECK(c, cfmm_pools_add_univ3(c, 1, price, gamma, A01, off, lower, liq));
    CHECK(c, cfmm_pools_add_weighted(c, 1, 3, R3, w3, gamma, A012));
    CHECK(c, cfmm_pools_add_curve(c, 1, 3, R3, gamma, A012, alpha, beta));
    CHECK(c, cfmm_pools_add_solidly(c, 1, R2, gamma, A12));

    const char* names[6] = {"product", "geomean", "univ3", "weighted", "curve", "solidly"};
    const int32_t cin[1] = {0}, cout[1] = {1};
    const double inf = INFINITY;
    for (int s = 0; s < 6; ++s) {
        double spot = -1, a = -1, out = -1, want = -2, back = -1, o2 = -1, zero = -1, zout = -1;
        CHECK(c, cfmm_quote_rate(c, s, 1, NULL, cin, cout, NULL, NULL, &spot));
        const double lim[1] = {0.9 * spot}, above[1] = {1.5 * spot};
        CHECK(c, cfmm_quote_to_rate(c, s, 1, NULL, cin, cout, lim, &a, &out));
        CHECK(c, cfmm_quote(c, s, 1, NULL, cin, cout, &a, &want));
        CHECK(c, cfmm_quote_rate(c, s, 1, NULL, cin, cout, &a, &o2, &back));
        CHECK(c, cfmm_quote_to_rate(c, s, 1, NULL, cin, cout, above, &zero, &zout));
        printf("%s: spot %.17g limit %.17g amount %.17g out %.17g rate there %.17g\n", names[s], spot, lim[0], a, out, back);
        if (!(a > 0) || memcmp(&out, &want, sizeof out)) return 3;
        if (!(fabs(back - lim[0]) <= 1e-12 * lim[0])) return 4;
        if (zero != 0.0 || signbit(zero) || zout != 0.0) return 5;
        double only = -1;
        CHECK(c, cfmm_quote_to_rate(c, s, 1, NULL, cin, cout, lim, &only, NULL));          /* amount_out may be NULL */
        if (memcmp(&only, &a, sizeof a)) return 6;

        /* the swap: as much as it takes; then the same limit with a margin finds nothing to do */
        double used = -1, got = -1, after = -1;
        int32_t st = -1;
        CHECK(c, cfmm_swap_limit(c, s, 1, NULL, cin, cout, &inf, lim, &used, &got, &st));
        CHECK(c, cfmm_quote_rate(c, s, 1, NULL, cin, cout, NULL, NULL, &after));
        printf("%s: swap_limit used %.17g out %.17g status %d, spot afterwards %.17g\n", names[s], used, got, st, after);
        if (st != CFMM_LIMIT_PARTIAL || memcmp(&used, &a, sizeof a) || memcmp(&got, &out, sizeof out)) return 7;
        if (!(fabs(after - lim[0]) <= 1e-12 * lim[0])) return 8;
        const double margin[1] = {lim[0] * (1 + 1e-9)};
        CHECK(c, cfmm_swap_limit(c, s, 1, NULL, cin, cout, &inf, margin, &used, &got, NULL)); /* status may be NULL */
        if (used != 0.0 || got != 0.0) return 9;
        const double small[1] = {1.0}, none[1] = {0.0};
        CHECK(c, cfmm_swap_limit(c, s, 1, NULL, cin, cout, small, none, &used, &got, &st));   /* limit 0: cfmm_swap */
        if (st != CFMM_LIMIT_FILLED || used != 1.0 || !(got > 0)) return 10;
    }
    CHECK(c, cfmm_quote_to_rate(c, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL));               /* count == 0: a no-op */
    CHECK(c, cfmm_swap_limit(c, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));

    /* refused before anything runs: the query is named, the outputs stay */
    const double bad[1] = {0.0}, one[1] = {1.0}, neg[1] = {-1.0};
    double keep = 7, keep2 = 7;
    int32_t keep3 = 7;
    if (cfmm_quote_to_rate(c, 0, 1, NULL, cin, cout, bad, &keep, &keep2) != CFMM_ERR_INVALID_ARG) return 11;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "cfmm_quote_to_rate: query 0: rate_limit must be finite and > 0") || keep != 7 || keep2 != 7) return 12;
    if (cfmm_swap_limit(c, 0, 1, NULL, cin, cout, one, neg, &keep, &keep2, &keep3) != CFMM_ERR_INVALID_ARG) return 13;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "cfmm_swap_limit: query 0: rate_limit must be finite and >= 0") || keep != 7 || keep2 != 7 || keep3 != 7) return 14;
    if (cfmm_swap_limit(c, 0, 1, NULL, cin, cout, &inf, bad, &keep, &keep2, &keep3) != CFMM_ERR_INVALID_ARG) return 15;   /* +inf without a limit */
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "cfmm_swap_limit: query 0: amount_in must be finite and >= 0") || keep != 7) return 16;
    cfmm_ctx_destroy(c);
    printf("abi_limit: ok\n");
    return 0;
}
