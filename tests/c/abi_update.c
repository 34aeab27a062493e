/* Plain-C client of the sparse pool-state updates (include/cfmm_amd.h: cfmm_pools_set_reserves / cfmm_pools_set_prices):
 * add -> set -> eval on one context against a context uploaded with the new state, bit for bit.  Built and run by
 * tests/test_gpu_pool_update.py on the MI355X box. */
#include <stdio.h>
#include <string.h>

#include "cfmm_amd.h"

#define CHECK(ctx, call)                                                                \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != CFMM_OK) {                                                           \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));        \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

int main(void)
{
    cfmm_ctx *a = NULL, *b = NULL;
    if (cfmm_ctx_create(0, 3, &a) != CFMM_OK || cfmm_ctx_create(0, 3, &b) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    const double R_old[6] = {1e6, 1e6, 1e3, 2e3, 5e2, 7e2}, R_new[6] = {1e6, 1e6, 1.5e3, 1.9e3, 6e2, 6.5e2};
    const double gamma[3] = {0.997, 1.0, 0.997};
    const int32_t Ai[6] = {0, 1, 0, 1, 1, 2};
    /* one UniV3 pool: ticks (20, 30], (10, 20], (0, 10] with the middle one empty */
    const double lt[3] = {30.0, 20.0, 10.0}, liq[3] = {1e6, 0.0, 2e6}, g3[1] = {0.997};
    const int32_t Ai3[2] = {0, 2};
    const int64_t off[2] = {0, 3};
    const double p_old[1] = {25.0}, p_new[1] = {15.0};
    CHECK(a, cfmm_pools_add_product(a, 3, R_old, gamma, Ai));
    CHECK(a, cfmm_pools_add_univ3(a, 1, p_old, g3, Ai3, off, lt, liq));
    CHECK(b, cfmm_pools_add_product(b, 3, R_new, gamma, Ai));
    CHECK(b, cfmm_pools_add_univ3(b, 1, p_new, g3, Ai3, off, lt, liq));

    const double v[3] = {2.0, 1.0, 0.05};
    double psi_a[3], psi_b[3], acc_a, acc_b;
    CHECK(a, cfmm_eval(a, v, psi_a, &acc_a));       /* the update goes behind an earlier sweep */
    const int64_t idx[3] = {2, 1, 2};               /* row 2 twice: the last value wins */
    const double R_set[6] = {9.0, 9.0, 1.5e3, 1.9e3, 6e2, 6.5e2};
    const int64_t idx3[1] = {0};
    CHECK(a, cfmm_pools_set_reserves(a, 0, 3, idx, R_set));
    CHECK(a, cfmm_pools_set_prices(a, 1, 1, idx3, p_new));
    CHECK(a, cfmm_pools_set_reserves(a, 0, 0, NULL, NULL));

    /* refused: nothing changes */
    const double R_bad[2] = {1.0, 0.0};
    if (cfmm_pools_set_reserves(a, 0, 1, idx3, R_bad) != CFMM_ERR_INVALID_ARG) return 3;
    printf("error message: %s\n", cfmm_last_error(a));
    if (cfmm_pools_set_prices(a, 0, 1, idx3, p_new) != CFMM_ERR_INVALID_ARG) return 4;
    printf("error message: %s\n", cfmm_last_error(a));
    double D[8], L[8];
    if (cfmm_get_trades(a, D, L) != CFMM_ERR_STATE) return 5;

    CHECK(a, cfmm_eval(a, v, psi_a, &acc_a));
    CHECK(b, cfmm_eval(b, v, psi_b, &acc_b));
    printf("updated: psi=[%.17g, %.17g, %.17g] acc=%.17g\n", psi_a[0], psi_a[1], psi_a[2], acc_a);
    printf("fresh:   psi=[%.17g, %.17g, %.17g] acc=%.17g\n", psi_b[0], psi_b[1], psi_b[2], acc_b);
    if (memcmp(psi_a, psi_b, sizeof psi_a) != 0 || memcmp(&acc_a, &acc_b, sizeof acc_a) != 0) return 6;
    double Ra[6], pa[1];
    CHECK(a, cfmm_get_reserves(a, 0, Ra));
    CHECK(a, cfmm_get_prices(a, 1, pa));
    if (memcmp(Ra, R_new, sizeof Ra) != 0 || pa[0] != p_new[0]) return 7;
    int64_t regrows = -1;
    CHECK(a, cfmm_get_option(a, "pool_update_regrows", &regrows));
    printf("pool_update_regrows = %lld\n", (long long)regrows);
    cfmm_ctx_destroy(a);
    cfmm_ctx_destroy(b);
    printf("ABI_UPDATE_OK\n");
    return acc_a != 0.0 ? 0 : 8;
}
