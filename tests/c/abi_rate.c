/* cfmm_quote_rate / cfmm_quote_path_rate from plain C: a market with one pool of each of the six kinds, one query per kind
 * (the amount out against cfmm_quote bit for bit, the rate against the slope of cfmm_quote around the amount), the spot-price
 * table (no amounts), a two-hop path against the product of its hops' rates, and the refusal of a bad query.  Exit code 0 =
 * everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_rate.h"

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
    const double amt[1] = {1000.0};
    double rates[6];
    for (int s = 0; s < 6; ++s) {
        double out = -1, rate = -1, want = -2, up, dn, spot = -1;
        const double au[1] = {amt[0] * (1 + 1e-6)}, ad[1] = {amt[0] * (1 - 1e-6)};
        CHECK(c, cfmm_quote_rate(c, s, 1, NULL, cin, cout, amt, &out, &rate));
        CHECK(c, cfmm_quote(c, s, 1, NULL, cin, cout, amt, &want));
        CHECK(c, cfmm_quote(c, s, 1, NULL, cin, cout, au, &up));
        CHECK(c, cfmm_quote(c, s, 1, NULL, cin, cout, ad, &dn));
        CHECK(c, cfmm_quote_rate(c, s, 1, NULL, cin, cout, NULL, NULL, &spot));   /* no amounts: the spot rate */
        const double slope = (up - dn) / (2e-6 * amt[0]);
        printf("%s: out %.17g rate %.17g slope %.9g spot %.17g\n", names[s], out, rate, slope, spot);
        if (memcmp(&out, &want, sizeof out)) return 3;
        if (!(fabs(rate - slope) <= 1e-4 * slope)) return 4;
        if (!(spot > rate && rate > 0)) return 5;
        rates[s] = rate;
    }
    CHECK(c, cfmm_quote_rate(c, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL));       /* count == 0: a no-op */

    /* a path: Product (token 0 -> 1), then Solidly (token 1 -> 2) */
    const int32_t n_hops[1] = {2}, hop_seg[2] = {0, 5}, hci[2] = {0, 0}, hco[2] = {1, 1};
    const int64_t hop_row[2] = {0, 0};
    double pout, prate, hout[2], hrate[2], qout, r1 = -1, o1 = -1;
    CHECK(c, cfmm_quote_path_rate(c, 1, 2, n_hops, hop_seg, hop_row, hci, hco, amt, &pout, &prate, hout, hrate));
    CHECK(c, cfmm_quote_path(c, 1, 2, n_hops, hop_seg, hop_row, hci, hco, amt, &qout, NULL));
    CHECK(c, cfmm_quote_rate(c, 5, 1, NULL, cin, cout, &hout[0], &o1, &r1));
    printf("path: out %.17g rate %.17g hops %.17g %.17g\n", pout, prate, hrate[0], hrate[1]);
    if (memcmp(&pout, &qout, sizeof pout) || memcmp(&o1, &pout, sizeof o1)) return 6;
    if (hrate[0] != rates[0] || hrate[1] != r1 || prate != hrate[0] * hrate[1]) return 7;

    /* refused before anything runs: the query is named, the outputs stay */
    const double bad[1] = {-1.0};
    double keep = 7, keep2 = 7;
    if (cfmm_quote_rate(c, 0, 1, NULL, cin, cout, bad, &keep, &keep2) != CFMM_ERR_INVALID_ARG) return 8;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "cfmm_quote_rate: query 0") || keep != 7 || keep2 != 7) return 9;
    cfmm_ctx_destroy(c);
    printf("abi_rate: ok\n");
    return 0;
}
