/* Plain-C client of cfmm_pools_set_ticks (include/cfmm_amd.h): a mint, a burn and a refused call on one context against a
 * context uploaded with the new ladders, bit for bit.  Built and run by tests/test_gpu_pool_ticks.py on the MI355X box. */
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
    /* two pools: ticks (20, 30], (10, 20], (0, 10] with the middle one empty; and a single tick (0, 8] */
    const double g[2] = {0.997, 1.0}, p[2] = {25.0, 3.0};
    const int32_t Ai[4] = {0, 2, 1, 2};
    const int64_t off_old[3] = {0, 3, 4};
    const double lt_old[4] = {30.0, 20.0, 10.0, 8.0}, lq_old[4] = {1e6, 0.0, 2e6, 1e6};
    /* pool 0 after a burn of its last tick and a mint into the empty one; pool 1 after mints on both sides of its price */
    const int64_t off_new[3] = {0, 2, 5};
    const double lt_new[5] = {30.0, 20.0, 8.0, 4.0, 2.0}, lq_new[5] = {1e6, 5e5, 1e6, 3e6, 1e5};
    CHECK(a, cfmm_pools_add_univ3(a, 2, p, g, Ai, off_old, lt_old, lq_old));
    CHECK(b, cfmm_pools_add_univ3(b, 2, p, g, Ai, off_new, lt_new, lq_new));

    const double v[3] = {2.0, 1.0, 0.05};
    double psi_a[3], psi_b[3], acc_a, acc_b;
    CHECK(a, cfmm_eval(a, v, psi_a, &acc_a));       /* the update goes behind an earlier sweep */
    /* rows in reverse order, as a CSR over the rows given */
    const int64_t idx[2] = {1, 0}, off_set[3] = {0, 3, 5};
    const double p_set[2] = {3.0, 25.0}, lt_set[5] = {8.0, 4.0, 2.0, 30.0, 20.0}, lq_set[5] = {1e6, 3e6, 1e5, 1e6, 5e5};
    CHECK(a, cfmm_pools_set_ticks(a, 0, 2, idx, p_set, off_set, lt_set, lq_set));
    CHECK(a, cfmm_pools_set_ticks(a, 0, 0, NULL, NULL, NULL, NULL, NULL));

    /* refused: nothing changes */
    const int64_t one[1] = {0}, off_bad[2] = {0, 2};
    const double p_bad[1] = {25.0}, lt_bad[2] = {20.0, 30.0}, lq_bad[2] = {1.0, 1.0};
    if (cfmm_pools_set_ticks(a, 0, 1, one, p_bad, off_bad, lt_bad, lq_bad) != CFMM_ERR_INVALID_ARG) return 3;
    printf("error message: %s\n", cfmm_last_error(a));
    double D[4], L[4];
    if (cfmm_get_trades(a, D, L) != CFMM_ERR_STATE) return 5;

    CHECK(a, cfmm_eval(a, v, psi_a, &acc_a));
    CHECK(b, cfmm_eval(b, v, psi_b, &acc_b));
    printf("updated: psi=[%.17g, %.17g, %.17g] acc=%.17g\n", psi_a[0], psi_a[1], psi_a[2], acc_a);
    printf("fresh:   psi=[%.17g, %.17g, %.17g] acc=%.17g\n", psi_b[0], psi_b[1], psi_b[2], acc_b);
    if (memcmp(psi_a, psi_b, sizeof psi_a) != 0 || memcmp(&acc_a, &acc_b, sizeof acc_a) != 0) return 6;
    int64_t regrows = -1;
    CHECK(a, cfmm_get_option(a, "pool_update_regrows", &regrows));
    printf("pool_update_regrows = %lld\n", (long long)regrows);
    cfmm_ctx_destroy(a);
    cfmm_ctx_destroy(b);
    printf("ABI_TICKS_OK\n");
    return acc_a != 0.0 ? 0 : 8;
}
