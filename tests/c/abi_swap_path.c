/* cfmm_swap_path from plain C: a market with one segment of every kind.  One path through all six kinds against the same
 * hops as cfmm_quote_path answers them and as six cfmm_swap calls move the pools on a twin; the same cycle twice in a batch with
 * a limit the second execution misses (status 1, nothing moved); a path whose last hop would empty a pool (status 2, NaN,
 * nothing moved, "swap_refused"); NULL for the optional arguments; a refused call (path and hops named, outputs and pools
 * untouched) and the state protocol (earlier trades are gone).  Exit code 0 = everything held. */
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

/* every reserve and price of the market, for "nothing moved" */
static int snapshot(cfmm_ctx* c, double* s)
{
    CHECK(c, cfmm_get_reserves(c, 0, s));
    CHECK(c, cfmm_get_reserves(c, 1, s + 6));
    CHECK(c, cfmm_get_prices(c, 2, s + 12));
    CHECK(c, cfmm_get_reserves(c, 3, s + 14));
    CHECK(c, cfmm_get_reserves(c, 4, s + 20));
    CHECK(c, cfmm_get_reserves(c, 5, s + 26));
    return 0;
}
#define SNAP 32

int main(void)
{
    cfmm_ctx *c = NULL, *t = NULL;
    if (cfmm_ctx_create(0, 3, &c) != CFMM_OK || cfmm_ctx_create(0, 3, &t) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    if (upload(c) || upload(t)) return 2;
    const double v[3] = {1.0, 1.3, 0.8};
    double D[64], L[64], s0[SNAP], s1[SNAP];
    CHECK(c, cfmm_find_arb(c, v));
    CHECK(c, cfmm_get_trades(c, D, L));

    /* one path through pool 1 of every segment, coin 0 for coin 1 at every hop */
    const int32_t six = 6, seg6[6] = {0, 1, 2, 3, 4, 5}, ci6[6] = {0, 0, 0, 0, 0, 0}, co6[6] = {1, 1, 1, 1, 1, 1};
    const int64_t row6[6] = {1, 1, 1, 1, 1, 1};
    const double a6 = 25.0, lim6 = 0.0;
    double q6 = -1, qh[6], o6 = -1, oh[6];
    int32_t st6 = -1;
    CHECK(t, cfmm_quote_path(t, 1, 6, &six, seg6, row6, ci6, co6, &a6, &q6, qh));
    CHECK(c, cfmm_swap_path(c, 1, 6, &six, seg6, row6, ci6, co6, &a6, &lim6, &o6, oh, &st6));
    printf("six kinds: quote %.17g executed %.17g status %d\n", q6, o6, (int)st6);
    if (st6 != CFMM_PATH_APPLIED || memcmp(&q6, &o6, sizeof q6) || memcmp(qh, oh, sizeof qh) || !(o6 > 0)) return 3;
    /* ... the earlier trades described the old market */
    if (cfmm_get_trades(c, D, L) != CFMM_ERR_STATE || !strstr(cfmm_last_error(c), "no materialised trades")) return 4;
    /* ... and the pools stand where six cfmm_swap calls leave the twin's */
    double x = a6;
    for (int k = 0; k < 6; ++k) {
        double out = -1;
        CHECK(t, cfmm_swap(t, seg6[k], 1, row6 + k, ci6 + k, co6 + k, &x, &out));
        if (memcmp(&out, oh + k, sizeof out)) return 5;
        x = out;
    }
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 6;

    /* the same two-hop cycle twice in one batch (hop-major arrays), the limit between the two results */
    const int32_t n2[2] = {2, 2}, segc[4] = {0, 0, 5, 5}, cic[4] = {0, 0, 1, 1}, coc[4] = {1, 1, 0, 0};
    const int64_t rowc[4] = {0, 0, 0, 0};
    const double ac[2] = {1e4, 1e4};
    const int32_t seg1[2] = {0, 5}, ci1[2] = {0, 1}, co1[2] = {1, 0};       /* the same cycle as a batch of one */
    double r1 = -1, q2 = -1, oc[2], limc[2];
    int32_t stc[2] = {-1, -1}, st1 = -1;
    CHECK(t, cfmm_swap_path(t, 1, 2, n2, seg1, rowc, ci1, co1, ac, NULL, &r1, NULL, &st1));
    CHECK(t, cfmm_quote_path(t, 1, 2, n2, seg1, rowc, ci1, co1, ac, &q2, NULL));
    if (st1 != CFMM_PATH_APPLIED || !(q2 < r1) || !(q2 > 0)) return 7;
    limc[0] = limc[1] = 0.5 * (r1 + q2);
    int64_t refused = -1, launches = -1;
    CHECK(c, cfmm_swap_path(c, 2, 2, n2, segc, rowc, cic, coc, ac, limc, oc, NULL, stc));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    CHECK(c, cfmm_get_option(c, "swap_launches", &launches));
    printf("cycle twice: %.17g status %d, then %.17g status %d (limit %.17g), swap_refused %lld, launches %lld\n", oc[0], (int)stc[0], oc[1],
           (int)stc[1], limc[0], (long long)refused, (long long)launches);
    if (stc[0] != CFMM_PATH_APPLIED || stc[1] != CFMM_PATH_BELOW_LIMIT || refused != 1 || launches != 2) return 8;
    if (memcmp(oc, &r1, sizeof r1) || memcmp(oc + 1, &q2, sizeof q2)) return 9;
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 10;                        /* only the first was executed */

    /* a path whose second hop would empty a Product pool: status 2, NaN, hop 0's pool untouched; no outputs but amount_out */
    const int32_t segr[2] = {1, 0}, cir[2] = {0, 0}, cor[2] = {1, 1};
    const int64_t rowr[2] = {0, 2};
    const double ar = 1e5;
    double orf = 0;
    /* (GeometricMean pool 0 gives a few 1e4 for 1e5; Product pool 2 is first set to a sliver, so that x/(R + x) rounds to 1) */
    const int64_t p2 = 2;
    const double tiny[2] = {1e-25, 1e-25};
    CHECK(c, cfmm_pools_set_reserves(c, 0, 1, &p2, tiny));
    if (snapshot(c, s0)) return 2;
    CHECK(c, cfmm_swap_path(c, 1, 2, n2, segr, rowr, cir, cor, &ar, NULL, &orf, NULL, NULL));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    if (snapshot(c, s1)) return 2;
    printf("refused path: %.17g, swap_refused %lld\n", orf, (long long)refused);
    if (!isnan(orf) || refused != 1 || memcmp(s0, s1, sizeof s0)) return 11;

    /* a refused call: path and hops are named, outputs and pools are untouched */
    const int32_t segd[2] = {0, 0};
    double keep = 7, keeph[2] = {7, 7};
    int32_t keeps = 7;
    if (cfmm_swap_path(c, 1, 2, n2, segd, rowc, cic, coc, ac, NULL, &keep, keeph, &keeps) != CFMM_ERR_INVALID_ARG) return 12;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strncmp(cfmm_last_error(c), "cfmm_swap_path:", 15) || !strstr(cfmm_last_error(c), "path 0, hops 0 and 1")) return 13;
    const double neg = -1.0;
    if (cfmm_swap_path(c, 1, 2, n2, seg1, rowc, ci1, co1, ac, &neg, &keep, keeph, &keeps) != CFMM_ERR_INVALID_ARG ||
        !strstr(cfmm_last_error(c), "path 0, hop 1: min_amount_out"))
        return 14;
    if (keep != 7 || keeph[0] != 7 || keeph[1] != 7 || keeps != 7) return 15;
    if (snapshot(c, s0)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 16;
    CHECK(c, cfmm_swap_path(c, 0, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));       /* count == 0: a no-op */
    cfmm_ctx_destroy(c);
    cfmm_ctx_destroy(t);
    printf("abi_swap_path: ok\n");
    return 0;
}
