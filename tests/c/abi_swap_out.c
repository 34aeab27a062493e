/* cfmm_swap_out and cfmm_swap_path_out from plain C: a market with one segment of every kind.  Single swaps: the answer is
 * cfmm_quote_out's, the pool gives exactly what was asked for, a limit one ulp short stops the swap (status 1, the would-be
 * quote, nothing moved), more than the pool holds is status 3 (+inf).  Paths: one path through all six kinds against
 * cfmm_quote_path_out's amounts and against six cfmm_swap_out calls on a twin (last hop first); the same path twice in a batch
 * with a limit the second execution exceeds; NULL for the optional arguments; a refused call (path and hops named, outputs and
 * pools untouched) and the state protocol (earlier trades are gone).  Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd.h"
#include "cfmm_amd_path_out.h"

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

    /* ---- cfmm_swap_out: Product pool 1 = {1e3, 2e3}, four swaps of the same row in one call */
    const int64_t rows[4] = {1, 1, 1, 1};
    const int32_t ci4[4] = {0, 0, 0, 0};
    const double want4[4] = {100.0, 2000.0, 50.0, 50.0};
    double q0 = -1, lim4[4], in4[4];
    int32_t st4[4] = {-1, -1, -1, -1};
    int64_t refused = -1, launches = -1;
    CHECK(t, cfmm_quote_out(t, 0, 1, rows, ci4, NULL, want4, &q0));
    /* the third swap would cost more than the first did per unit; its limit is the first's cost: over the limit */
    lim4[0] = q0; lim4[1] = 1e300; lim4[2] = 0.25 * q0; lim4[3] = 1e300;
    CHECK(c, cfmm_swap_out(c, 0, 4, rows, ci4, NULL, want4, lim4, in4, st4));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    CHECK(c, cfmm_get_option(c, "swap_launches", &launches));
    printf("swap_out: in %.17g %.17g %.17g %.17g status %d %d %d %d, swap_refused %lld, launches %lld\n", in4[0], in4[1], in4[2], in4[3],
           (int)st4[0], (int)st4[1], (int)st4[2], (int)st4[3], (long long)refused, (long long)launches);
    if (memcmp(&q0, in4, sizeof q0)) return 3;                        /* a limit equal to the quote is met */
    if (st4[0] != CFMM_SWAP_APPLIED || st4[1] != CFMM_SWAP_UNOBTAINABLE || st4[2] != CFMM_SWAP_OVER_LIMIT || st4[3] != CFMM_SWAP_APPLIED) return 4;
    if (!isinf(in4[1]) || memcmp(in4 + 2, in4 + 3, sizeof(double)) || !(in4[2] > 0.25 * q0) || refused != 2 || launches != 4) return 5;
    if (cfmm_get_trades(c, D, L) != CFMM_ERR_STATE || !strstr(cfmm_last_error(c), "no materialised trades")) return 6;
    if (snapshot(c, s0)) return 2;
    {   /* the pool gave exactly 100 and 50, and took γ·in with each operation rounded on its own */
        const double r0 = (1e3 + in4[0]) + in4[3], r1 = (2e3 - 100.0) - 50.0;   /* γ of pool 1 is 1.0 */
        if (s0[2] != r0 || s0[3] != r1) return 7;
    }
    CHECK(t, cfmm_swap_out(t, 0, 1, rows, ci4, NULL, want4, NULL, in4, NULL));           /* limits and statuses as NULL */
    CHECK(t, cfmm_swap_out(t, 0, 1, rows, ci4, NULL, want4 + 3, NULL, in4 + 3, NULL));
    if (snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 8;

    /* ---- cfmm_swap_path_out: one path through pool 1 of every segment, coin 0 for coin 1 at every hop */
    const int32_t six = 6, seg6[6] = {0, 1, 2, 3, 4, 5}, ci6[6] = {0, 0, 0, 0, 0, 0}, co6[6] = {1, 1, 1, 1, 1, 1};
    const int64_t row6[6] = {1, 1, 1, 1, 1, 1};
    const double w6 = 5.0, lim6 = 1e300;
    double q6 = -1, qh[6], a6 = -1, ah[6];
    int32_t st6 = -1;
    CHECK(t, cfmm_quote_path_out(t, 1, 6, &six, seg6, row6, ci6, co6, &w6, &q6, qh));
    CHECK(c, cfmm_swap_path_out(c, 1, 6, &six, seg6, row6, ci6, co6, &w6, &lim6, &a6, ah, &st6));
    printf("six kinds: quote %.17g executed %.17g status %d\n", q6, a6, (int)st6);
    if (st6 != CFMM_SWAP_APPLIED || memcmp(&q6, &a6, sizeof q6) || memcmp(qh, ah, sizeof qh) || !(a6 > 0) || !isfinite(a6)) return 9;
    /* ... and the pools stand where six cfmm_swap_out calls leave the twin's, the last hop first */
    double y = w6;
    for (int k = 5; k >= 0; --k) {
        double in = -1;
        int32_t st = -1;
        CHECK(t, cfmm_swap_out(t, seg6[k], 1, row6 + k, ci6 + k, co6 + k, &y, NULL, &in, &st));
        if (st != CFMM_SWAP_APPLIED || memcmp(&in, ah + k, sizeof in)) return 10;
        y = in;
    }
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 11;

    /* the same two-hop path twice in one batch (hop-major arrays), the limit between the two costs */
    const int32_t n2[2] = {2, 2}, segc[4] = {0, 0, 5, 5}, cic[4] = {0, 0, 1, 1}, coc[4] = {1, 1, 0, 0};
    const int64_t rowc[4] = {0, 0, 0, 0};
    const double wc[2] = {1e3, 1e3};
    const int32_t seg1[2] = {0, 5}, ci1[2] = {0, 1}, co1[2] = {1, 0};       /* the same path as a batch of one */
    double r1 = -1, q2 = -1, ac[2], limc[2];
    int32_t stc[2] = {-1, -1}, st1 = -1;
    CHECK(t, cfmm_swap_path_out(t, 1, 2, n2, seg1, rowc, ci1, co1, wc, NULL, &r1, NULL, &st1));
    CHECK(t, cfmm_quote_path_out(t, 1, 2, n2, seg1, rowc, ci1, co1, wc, &q2, NULL));
    if (st1 != CFMM_SWAP_APPLIED || !(q2 > r1) || !(r1 > 0) || !isfinite(q2)) return 12;   /* the second costs more */
    limc[0] = limc[1] = 0.5 * (r1 + q2);
    CHECK(c, cfmm_swap_path_out(c, 2, 2, n2, segc, rowc, cic, coc, wc, limc, ac, NULL, stc));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    CHECK(c, cfmm_get_option(c, "swap_launches", &launches));
    printf("path twice: %.17g status %d, then %.17g status %d (limit %.17g), swap_refused %lld, launches %lld\n", ac[0], (int)stc[0], ac[1],
           (int)stc[1], limc[0], (long long)refused, (long long)launches);
    if (stc[0] != CFMM_SWAP_APPLIED || stc[1] != CFMM_SWAP_OVER_LIMIT || refused != 1 || launches != 2) return 13;
    if (memcmp(ac, &r1, sizeof r1) || memcmp(ac + 1, &q2, sizeof q2)) return 14;
    if (snapshot(c, s0) || snapshot(t, s1)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 15;                        /* only the first was executed */

    /* a path whose first hop's pool cannot give what the second asks of it: status 3, +inf, nothing moved */
    const int32_t segr[2] = {0, 1}, cir[2] = {0, 0}, cor[2] = {1, 1};
    const int64_t rowr[2] = {2, 0};
    const double wr = 10.0;
    double inr = 0, hr[2] = {0, 0};
    int32_t str = -1;
    const int64_t p2 = 2;
    const double tiny[2] = {1e-25, 1e-25};
    CHECK(c, cfmm_pools_set_reserves(c, 0, 1, &p2, tiny));
    if (snapshot(c, s0)) return 2;
    CHECK(c, cfmm_swap_path_out(c, 1, 2, n2, segr, rowr, cir, cor, &wr, NULL, &inr, hr, &str));
    CHECK(c, cfmm_get_option(c, "swap_refused", &refused));
    if (snapshot(c, s1)) return 2;
    printf("unobtainable path: %.17g (hops %.17g %.17g) status %d, swap_refused %lld\n", inr, hr[0], hr[1], (int)str, (long long)refused);
    if (str != CFMM_SWAP_UNOBTAINABLE || !isinf(inr) || !isinf(hr[0]) || !(hr[1] > 0) || !isfinite(hr[1]) || refused != 1 || memcmp(s0, s1, sizeof s0))
        return 16;

    /* a refused call: path and hops are named, outputs and pools are untouched */
    const int32_t segd[2] = {0, 0};
    double keep = 7, keeph[2] = {7, 7};
    int32_t keeps = 7;
    if (cfmm_swap_path_out(c, 1, 2, n2, segd, rowc, cic, coc, wc, NULL, &keep, keeph, &keeps) != CFMM_ERR_INVALID_ARG) return 17;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strncmp(cfmm_last_error(c), "cfmm_swap_path_out:", 19) || !strstr(cfmm_last_error(c), "path 0, hops 0 and 1")) return 18;
    const double neg = -1.0;
    if (cfmm_swap_path_out(c, 1, 2, n2, seg1, rowc, ci1, co1, wc, &neg, &keep, keeph, &keeps) != CFMM_ERR_INVALID_ARG ||
        !strstr(cfmm_last_error(c), "path 0, hop 0: max_amount_in"))
        return 19;
    if (cfmm_swap_out(c, 0, 1, rows, ci4, NULL, want4, &neg, &keep, &keeps) != CFMM_ERR_INVALID_ARG ||
        strncmp(cfmm_last_error(c), "cfmm_swap_out:", 14) || !strstr(cfmm_last_error(c), "query 0: max_amount_in"))
        return 20;
    if (keep != 7 || keeph[0] != 7 || keeph[1] != 7 || keeps != 7) return 21;
    if (snapshot(c, s0)) return 2;
    if (memcmp(s0, s1, sizeof s0)) return 22;
    CHECK(c, cfmm_swap_path_out(c, 0, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */
    CHECK(c, cfmm_swap_out(c, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
    cfmm_ctx_destroy(c);
    cfmm_ctx_destroy(t);
    printf("abi_swap_out: ok\n");
    return 0;
}
