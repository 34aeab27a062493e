/* cfmm_swap_order / cfmm_swap_order_out from plain C: abi_swap_path.c's market with one segment of every kind.  One order of three
 * paths against cfmm_swap_path on the same flat paths on a twin (amounts, the serial total, the pools); the same order twice in a
 * batch with a limit on the total that the second execution misses (status 1, its paths held, nothing moved); an order one of
 * whose paths would empty a pool (status 2, NaN total, the sibling path held, nothing moved, "swap_refused"); the exact-output
 * twin against cfmm_swap_path_out; a refused call (the order and its paths named, outputs and pools untouched).  Exit code 0 =
 * everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_order.h"

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

    /* one order of three paths over pool 1 of five segments (hop-major arrays, 3 paths, 2 hops): Product -> weighted,
     * GeometricMean -> Curve, Solidly alone; coin 0 for coin 1 at every hop */
    const int32_t nh3[3] = {2, 2, 1}, seg3[6] = {0, 1, 5, 3, 4, 0}, ci3[6] = {0, 0, 0, 0, 0, 0}, co3[6] = {1, 1, 1, 1, 1, 0};
    const int64_t row3[6] = {1, 1, 1, 1, 1, 0}, first1[2] = {0, 3};
    const double a3[3] = {20.0, 15.0, 10.0}, lim0 = 0.0;
    double want[3], wanth[6], o3[3], oh[6], tot = -1;
    int32_t wst[3], pst[3] = {-1, -1, -1}, st = -1;
    CHECK(t, cfmm_swap_path(t, 3, 2, nh3, seg3, row3, ci3, co3, a3, NULL, want, wanth, wst));
    CHECK(c, cfmm_swap_order(c, 1, first1, 3, 2, nh3, seg3, row3, ci3, co3, a3, &lim0, o3, oh, &tot, pst, &st));
    const double sum3 = (want[0] + want[1]) + want[2];
    printf("three paths: total %.17g (serial sum %.17g) status %d\n", tot, sum3, (int)st);
    if (st != CFMM_ORDER_APPLIED || pst[0] != CFMM_PATH_APPLIED || pst[1] != CFMM_PATH_APPLIED || pst[2] != CFMM_PATH_APPLIED) return 3;
    if (wst[0] != CFMM_PATH_APPLIED || wst[1] != CFMM_PATH_APPLIED || wst[2] != CFMM_PATH_APPLIED) return 3;
    if (memcmp(o3, want, sizeof want) || memcmp(oh, wanth, 5 * sizeof(double)) || !isnan(oh[5]) || memcmp(&tot, &sum3, sizeof tot) || !(tot > 0)) return 4;
    /* ... the earlier trades described the old market, and the pools stand where cfmm_swap_path leaves the twin's */
    if (cfmm_get_trades(c, D, L) != CFMM_ERR_STATE || !strstr(cfmm_last_error(c), "no materialised trades")) return 5;
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 6;

    /* the same order of two one-hop paths twice in one batch, the limit between the two totals */
    const int32_t nh1[4] = {1, 1, 1, 1}, segc[4] = {0, 5, 0, 5}, cic[4] = {0, 0, 0, 0}, coc[4] = {1, 1, 1, 1};
    const int64_t rowc[4] = {0, 0, 0, 0}, first2[3] = {0, 2, 4};
    const double ac[4] = {1e4, 1e4, 1e4, 1e4};
    double r1[2], q2[2], oc[4], totc[2], limc[2], t1 = -1;
    int32_t stc[2] = {-1, -1}, pstc[4], st1 = -1;
    CHECK(t, cfmm_swap_order(t, 1, first2, 2, 1, nh1, segc, rowc, cic, coc, ac, NULL, r1, NULL, &t1, NULL, &st1));
    CHECK(t, cfmm_quote_path(t, 2, 1, nh1, segc, rowc, cic, coc, ac, q2, NULL));
    const double t2 = q2[0] + q2[1];
    if (st1 != CFMM_ORDER_APPLIED || !(t2 < t1) || !(t2 > 0)) return 7;
    limc[0] = limc[1] = 0.5 * (t1 + t2);
    int64_t refused = -1, launches = -1;
    CHECK(c, cfmm_swap_order(c, 2, first2, 4, 1, nh1, segc, rowc, cic, coc, ac, limc, oc, NULL, totc, pstc, stc));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    CHECK(c, cfmm_get_option(c, "swap_launches", &launches));
    printf("order twice: %.17g status %d, then %.17g status %d (limit %.17g), swap_refused %lld, launches %lld\n", totc[0], (int)stc[0], totc[1],
           (int)stc[1], limc[0], (long long)refused, (long long)launches);
    if (stc[0] != CFMM_ORDER_APPLIED || stc[1] != CFMM_ORDER_LIMIT || refused != 1 || launches != 2) return 8;
    if (pstc[0] != CFMM_PATH_APPLIED || pstc[1] != CFMM_PATH_APPLIED || pstc[2] != CFMM_ORDER_PATH_HELD || pstc[3] != CFMM_ORDER_PATH_HELD) return 8;
    if (memcmp(totc, &t1, sizeof t1) || memcmp(totc + 1, &t2, sizeof t2) || memcmp(oc, r1, sizeof r1) || memcmp(oc + 2, q2, sizeof q2)) return 9;
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 10;                        /* only the first was executed */

    /* an order whose second path would empty a Product pool at its second hop: status 2, NaN total, the sibling held */
    const int32_t nhr[2] = {1, 2}, segr[4] = {3, 1, 0, 0}, cir[4] = {0, 0, 0, 0}, cor[4] = {1, 1, 0, 1};
    const int64_t rowr[4] = {0, 0, 0, 2}, firstr[2] = {0, 2};
    const double ar[2] = {5.0, 1e5};
    double orf[2] = {0, 0}, totr = 0;
    int32_t pstr[2] = {-1, -1}, str = -1;
    /* (GeometricMean pool 0 gives a few 1e4 for 1e5; Product pool 2 is first set to a sliver, so that x/(R + x) rounds to 1) */
    const int64_t p2 = 2;
    const double tiny[2] = {1e-25, 1e-25};
    CHECK(c, cfmm_pools_set_reserves(c, 0, 1, &p2, tiny));
    if (snapshot(c, s0)) return 2;
    CHECK(c, cfmm_swap_order(c, 1, firstr, 2, 2, nhr, segr, rowr, cir, cor, ar, NULL, orf, NULL, &totr, pstr, &str));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    if (snapshot(c, s1)) return 2;
    printf("refused order: total %.17g, sibling %.17g, swap_refused %lld\n", totr, orf[0], (long long)refused);
    if (str != CFMM_ORDER_REFUSED || !isnan(totr) || !isnan(orf[1]) || !(orf[0] > 0) || refused != 1 || memcmp(s0, s1, sizeof s0)) return 11;
    if (pstr[0] != CFMM_ORDER_PATH_HELD || pstr[1] != CFMM_PATH_REFUSED) return 11;

    /* exact output: one order of two paths, each asked for half of what 10 of its first coin yields */
    const int32_t nho[2] = {2, 1}, sego[4] = {1, 3, 4, 0}, cio[4] = {0, 0, 0, 0}, coo[4] = {1, 1, 1, 0};
    const int64_t rowo[4] = {1, 1, 1, 0}, firsto[2] = {0, 2};
    const double ten[2] = {10.0, 10.0};
    double fwd[2], wanto[2], costw[2], costh[4], cost[2], costgh[4], toto = -1;
    int32_t stw[2], psto[2], sto = -1;
    CHECK(t, cfmm_pools_set_reserves(t, 0, 1, &p2, tiny));
    CHECK(t, cfmm_quote_path(t, 2, 2, nho, sego, rowo, cio, coo, ten, fwd, NULL));
    wanto[0] = 0.5 * fwd[0];
    wanto[1] = 0.5 * fwd[1];
    CHECK(t, cfmm_swap_path_out(t, 2, 2, nho, sego, rowo, cio, coo, wanto, NULL, costw, costh, stw));
    const double sumo = costw[0] + costw[1], maxo = sumo;
    CHECK(c, cfmm_swap_order_out(c, 1, firsto, 2, 2, nho, sego, rowo, cio, coo, wanto, &maxo, cost, costgh, &toto, psto, &sto));
    printf("exact output: total_in %.17g (serial sum %.17g) status %d\n", toto, sumo, (int)sto);
    if (sto != CFMM_ORDER_APPLIED || stw[0] != CFMM_SWAP_APPLIED || stw[1] != CFMM_SWAP_APPLIED || psto[0] != CFMM_PATH_APPLIED || psto[1] != CFMM_PATH_APPLIED) return 12;
    if (memcmp(cost, costw, sizeof cost) || memcmp(costgh, costh, 3 * sizeof(double)) || memcmp(&toto, &sumo, sizeof toto) || !(toto > 0)) return 13;
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 14;

    /* a refused call: the order and its paths are named, outputs and pools are untouched */
    const int32_t segd[2] = {0, 0};
    double keep[2] = {7, 7}, keept = 7;
    int32_t keeps = 7, keepp[2] = {7, 7};
    if (cfmm_swap_order(c, 1, firsto, 2, 1, nh1, segd, rowc, cic, coc, ac, NULL, keep, NULL, &keept, keepp, &keeps) != CFMM_ERR_INVALID_ARG) return 15;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strncmp(cfmm_last_error(c), "cfmm_swap_order:", 16) || !strstr(cfmm_last_error(c), "order 0: paths 0 and 1 share pool (segment 0, row 0)")) return 16;
    const double neg = -1.0;
    if (cfmm_swap_order(c, 1, firsto, 2, 1, nh1, segc, rowc, cic, coc, ac, &neg, keep, NULL, &keept, keepp, &keeps) != CFMM_ERR_INVALID_ARG ||
        !strstr(cfmm_last_error(c), "order 0: min_total_out"))
        return 17;
    if (keep[0] != 7 || keep[1] != 7 || keept != 7 || keeps != 7 || keepp[0] != 7 || keepp[1] != 7) return 18;
    if (snapshot(c, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 19;
    CHECK(c, cfmm_swap_order(c, 0, NULL, 0, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */
    cfmm_ctx_destroy(c);
    cfmm_ctx_destroy(t);
    printf("abi_swap_order: ok\n");
    return 0;
}
