/* cfmm_find_disjoint_paths_out from plain C: three ProductTwoCoin pools 0 -> 1 of different depth and a two-hop detour
 * 0 -> 2 -> 1.  One call finds the four routes that can each give 10 000 of token 1 -- no pool twice, cheapest first, slot 0
 * cfmm_find_path_out's answer -- in the arrays cfmm_quote_path_out takes slot by slot; a second query for a token no pool holds
 * finds nothing (+inf); a third wants more than any path gives alone; two refused calls name the entry.
 * Exit code 0 = everything held. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cfmm_amd_find_disjoint_out.h"

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CFMM_OK) {                                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cfmm_last_error(ctx));         \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

enum { N = 3, K = 6, H = 3 };   /* queries, max_paths, max_hops */

/* (hop k of path r of query q of n) */
static int at_hop(int r, int k, int q) { return (r * H + k) * N + q; }

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 4, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    /* pools 0 .. 2 trade token 0 for token 1; pools 3 and 4 are the detour 0 -> 2 -> 1; token 3 is held by no pool */
    const double R[10] = {1.0e5, 1.0e5, 5.0e4, 5.0e4, 2.0e4, 2.0e4, 8.0e4, 8.0e4, 8.0e4, 8.0e4};
    const double gamma[5] = {0.997, 0.999, 0.997, 0.997, 0.997};
    const int32_t Ai[10] = {0, 1, 0, 1, 0, 1, 0, 2, 2, 1};
    CHECK(c, cfmm_pools_add_product(c, 5, R, gamma, Ai));

    const int32_t tin[N] = {0, 0, 0}, tout[N] = {1, 3, 1};
    const double amount[N] = {1.0e4, 1.0e4, 1.5e5};   /* (query 2: more than the deepest pool holds) */
    int32_t n_paths[N], n_hops[K * N], status[K * N], seg[K * H * N], cin[K * H * N], cout[K * H * N];
    int64_t row[K * H * N];
    double out[K * N];
    CHECK(c, cfmm_find_disjoint_paths_out(c, N, K, H, tin, tout, amount, n_paths, out, n_hops, status, seg, row, cin, cout));
    printf("query 0: %d paths, query 1: %d paths\n", (int)n_paths[0], (int)n_paths[1]);
    if (n_paths[0] != 4 || n_paths[1] != 0 || n_paths[2] != 0) return 3;
    int seen[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < K; ++r) {
        const int at = r * N;
        printf("path %d: status %d, %d hops, %.17g in, rows", r, (int)status[at], (int)n_hops[at], out[at]);
        for (int k = 0; k < H; ++k) printf(" %lld", (long long)row[at_hop(r, k, 0)]);
        printf("\n");
        if (status[at + 1] != CFMM_FOUND_NONE || n_hops[at + 1] != 0 || !(isinf(out[at + 1]) && out[at + 1] > 0)) return 4;   /* query 1: nothing, everywhere */
        if (status[at + 2] != CFMM_FOUND_NONE || !(isinf(out[at + 2]) && out[at + 2] > 0)) return 4;                            /* query 2: no path gives it alone */
        if (r >= 4) {
            if (status[at] != CFMM_FOUND_NONE || n_hops[at] != 0 || !isinf(out[at]) || row[at_hop(r, 0, 0)] != -1 || seg[at_hop(r, 0, 0)] != -1) return 5;
            continue;
        }
        if (status[at] != CFMM_FOUND || (r > 0 && !(out[at] >= out[at - N]))) return 6;
        for (int k = 0; k < n_hops[at]; ++k) {
            const int64_t p = row[at_hop(r, k, 0)];
            if (p < 0 || p > 4 || seg[at_hop(r, k, 0)] != 0 || seen[p]++) return 7;                      /* no pool twice */
        }
    }
    for (int p = 0; p < 5; ++p)
        if (!seen[p]) return 8;                                                                          /* every pool is on some path */
    if (row[0] != 0 || n_hops[0] != 1 || n_hops[2 * N] != 2) return 9;                                   /* cheapest first; the detour is third */
    /* slot 0 is cfmm_find_path_out's answer, and slot r quotes to its amount bit for bit */
    double one[N], back[1];
    int32_t nh1[N], st1[N], seg1[H * N], ci1[H * N], co1[H * N];
    int64_t row1[H * N];
    CHECK(c, cfmm_find_path_out(c, N, H, tin, tout, amount, one, nh1, seg1, row1, ci1, co1, st1));
    if (memcmp(one, out, sizeof one) || memcmp(nh1, n_hops, sizeof nh1) || memcmp(row1, row, sizeof row1) || memcmp(st1, status, sizeof st1)) return 10;
    for (int r = 0; r < 4; ++r) {   /* (query 0's hops of slot r, gathered: cfmm_quote_path_out refuses query 1's empty path) */
        int32_t qs[H], qi[H], qo[H];
        int64_t qr[H];
        for (int k = 0; k < H; ++k) {
            qs[k] = seg[at_hop(r, k, 0)];
            qr[k] = row[at_hop(r, k, 0)];
            qi[k] = cin[at_hop(r, k, 0)];
            qo[k] = cout[at_hop(r, k, 0)];
        }
        CHECK(c, cfmm_quote_path_out(c, 1, H, &n_hops[r * N], qs, qr, qi, qo, amount, back, NULL));
        if (memcmp(back, &out[r * N], sizeof(double))) return 11;
    }
    CHECK(c, cfmm_find_disjoint_paths_out(c, 0, K, H, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));   /* count == 0: a no-op */

    /* refused before anything runs: the outputs stay */
    int32_t keep[N] = {7, 7, 7};
    if (cfmm_find_disjoint_paths_out(c, N, CFMM_MAX_SPLIT_PATHS + 1, H, tin, tout, amount, keep, out, n_hops, status, seg, row, cin, cout) != CFMM_ERR_INVALID_ARG) return 12;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strcmp(cfmm_last_error(c), "cfmm_find_disjoint_paths_out: max_paths must be 1 .. 8 (got 9)")) return 13;
    const int32_t bad_out[N] = {1, 4, 1};
    if (cfmm_find_disjoint_paths_out(c, N, K, H, tin, bad_out, amount, keep, out, n_hops, status, seg, row, cin, cout) != CFMM_ERR_INVALID_ARG) return 14;
    printf("error message: %s\n", cfmm_last_error(c));
    if (strcmp(cfmm_last_error(c), "cfmm_find_disjoint_paths_out: query 1: token_out 4 out of range (the market has 4 tokens)")) return 15;
    if (keep[0] != 7 || keep[1] != 7 || keep[2] != 7) return 16;
    cfmm_ctx_destroy(c);
    printf("abi_find_disjoint_out: ok\n");
    return 0;
}
