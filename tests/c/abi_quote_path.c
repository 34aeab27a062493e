/* cfmm_quote_path / cfmm_quote_path_out from plain C: a two-segment market (three ProductTwoCoin pools, two 3-coin weighted
 * pools), three paths of 2, 1 and 3 hops across both segments in the hop-major layout, both directions against the chain of
 * cfmm_quote / cfmm_quote_out calls (bit for bit) and, on the product hop, against the closed form; the NaN of the unused hop
 * slots, +inf from an infeasible hop to the first, and one refused call that names path and hop.  Exit code 0 = everything held. */
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

enum { P = 3, H = 3 };   /* paths, max_hops */

int main(void)
{
    cfmm_ctx* c = NULL;
    if (cfmm_ctx_create(0, 4, &c) != CFMM_OK) {
        fprintf(stderr, "cfmm_ctx_create: %s\n", cfmm_last_error(NULL));
        return 2;
    }
    const double R[6] = {1e6, 1e6, 1e3, 2e3, 5e2, 7e2};
    const double gamma[3] = {0.997, 1.0, 0.997};
    const int32_t Ai[6] = {0, 1, 0, 1, 1, 2};
    CHECK(c, cfmm_pools_add_product(c, 3, R, gamma, Ai));                        /* segment 0 */
    const double Rw[6] = {4e3, 5e3, 6e3, 1e2, 2e2, 3e2}, w[6] = {0.2, 0.3, 0.5, 1.0, 1.0, 2.0};
    const double gw[2] = {0.997, 0.99};
    const int32_t Aw[6] = {0, 1, 2, 1, 2, 3};
    CHECK(c, cfmm_pools_add_weighted(c, 2, 3, Rw, w, gw, Aw));                   /* segment 1 */
    if (cfmm_segment_count(c) != 2) return 3;

    /* hop-major: entry k*P + p.  Path 0: product row 1 (0 -> 1), weighted row 0 (2 -> 0).  Path 1: weighted row 1 (0 -> 1).
     * Path 2: product row 0 (1 -> 0), product row 2 (0 -> 1), weighted row 0 (1 -> 2).  Unused slots hold garbage. */
    const int32_t n_hops[P] = {2, 1, 3};
    const int32_t seg[H * P] = {0, 1, 0, /**/ 1, -9, 0, /**/ 77, 77, 1};
    const int64_t row[H * P] = {1, 1, 0, /**/ 0, 99, 2, /**/ -1, -1, 0};
    const int32_t cin[H * P] = {0, 0, 1, /**/ 2, 5, 0, /**/ 5, 5, 1};
    const int32_t cout[H * P] = {1, 1, 0, /**/ 0, 5, 1, /**/ 5, 5, 2};
    const double amount_in[P] = {10.0, 3.0, 2500.0};
    double out[P], hop_out[H * P], out2[P];
    CHECK(c, cfmm_quote_path(c, P, H, n_hops, seg, row, cin, cout, amount_in, out, hop_out));

    /* the chain through cfmm_quote, one call per hop */
    for (int p = 0; p < P; ++p) {
        double x = amount_in[p];
        for (int k = 0; k < H; ++k) {
            const int at = k * P + p;
            if (k >= n_hops[p]) {
                if (!isnan(hop_out[at])) return 4;                                /* unused slots are NaN */
                continue;
            }
            double y;
            CHECK(c, cfmm_quote(c, seg[at], 1, &row[at], &cin[at], &cout[at], &x, &y));
            printf("path %d hop %d: segment %d row %lld: %.17g -> %.17g\n", p, k, seg[at], (long long)row[at], x, hop_out[at]);
            if (memcmp(&y, &hop_out[at], sizeof y)) return 5;
            x = y;
        }
        if (memcmp(&x, &out[p], sizeof x)) return 6;
    }
    /* the product hop of path 0 against the closed form */
    if (hop_out[0] != R[3] * ((gamma[1] * 10.0) / (R[2] + gamma[1] * 10.0))) return 7;
    CHECK(c, cfmm_quote_path(c, P, H, n_hops, seg, row, cin, cout, amount_in, out2, NULL));      /* hop_out may be NULL */
    if (memcmp(out, out2, sizeof out)) return 8;
    CHECK(c, cfmm_quote_path(c, 0, H, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));          /* count == 0: a no-op */

    /* exact output: half of what came out, walked backwards; then the chain through cfmm_quote_out */
    double want[P], in[P], hop_in[H * P];
    for (int p = 0; p < P; ++p) want[p] = 0.5 * out[p];
    CHECK(c, cfmm_quote_path_out(c, P, H, n_hops, seg, row, cin, cout, want, in, hop_in));
    for (int p = 0; p < P; ++p) {
        double y = want[p];
        for (int k = H - 1; k >= 0; --k) {
            const int at = k * P + p;
            if (k >= n_hops[p]) {
                if (!isnan(hop_in[at])) return 9;
                continue;
            }
            double x;
            CHECK(c, cfmm_quote_out(c, seg[at], 1, &row[at], &cin[at], &cout[at], &y, &x));
            printf("path %d hop %d backwards: wanted %.17g -> tender %.17g\n", p, k, y, hop_in[at]);
            if (memcmp(&x, &hop_in[at], sizeof x)) return 10;
            y = x;
        }
        if (memcmp(&y, &in[p], sizeof y) || memcmp(&in[p], &hop_in[p], sizeof y)) return 11;
        if (!(in[p] < amount_in[p])) return 12;                                   /* half the output costs less than the input */
    }
    /* path 2 asked for the whole reserve of its last pool's coin out: that hop, every earlier one and the answer are +inf */
    const double too_much[P] = {want[0], want[1], Rw[2]};
    CHECK(c, cfmm_quote_path_out(c, P, H, n_hops, seg, row, cin, cout, too_much, out2, hop_in));
    printf("beyond the reserve: %.17g %.17g %.17g %.17g\n", out2[2], hop_in[0 * P + 2], hop_in[1 * P + 2], hop_in[2 * P + 2]);
    if (out2[0] != in[0] || out2[1] != in[1]) return 13;
    if (!isinf(out2[2]) || out2[2] < 0 || !isinf(hop_in[2]) || !isinf(hop_in[P + 2]) || !isinf(hop_in[2 * P + 2])) return 14;

    /* refused before anything runs: path and hop are named, the outputs stay */
    int64_t bad_row[H * P];
    memcpy(bad_row, row, sizeof row);
    bad_row[1 * P + 2] = 3;                                                       /* path 2, hop 1: segment 0 has rows 0..2 */
    double keep[P] = {7, 7, 7}, keep_hops[H * P];
    for (int i = 0; i < H * P; ++i) keep_hops[i] = 7;
    if (cfmm_quote_path(c, P, H, n_hops, seg, bad_row, cin, cout, amount_in, keep, keep_hops) != CFMM_ERR_INVALID_ARG) return 15;
    printf("error message: %s\n", cfmm_last_error(c));
    if (!strstr(cfmm_last_error(c), "path 2, hop 1: row 3") || strncmp(cfmm_last_error(c), "cfmm_quote_path:", 16)) return 16;
    for (int i = 0; i < P; ++i)
        if (keep[i] != 7) return 17;
    for (int i = 0; i < H * P; ++i)
        if (keep_hops[i] != 7) return 17;
    if (cfmm_quote_path_out(c, P, CFMM_MAX_PATH_HOPS + 1, n_hops, seg, row, cin, cout, want, keep, NULL) != CFMM_ERR_INVALID_ARG) return 18;
    if (strncmp(cfmm_last_error(c), "cfmm_quote_path_out:", 20)) return 19;
    if (cfmm_quote_path_dev(c, -1, H, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != CFMM_ERR_INVALID_ARG) return 20;
    cfmm_ctx_destroy(c);
    printf("abi_quote_path: ok\n");
    return 0;
}
