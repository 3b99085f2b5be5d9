/* gram_ref.c -- the sequential restatement of the topic-map contract of include/mvhdp.h (mvhdp_topic_gram): plain loops, libm's fma and
 * sqrt, one cell at a time.  Test infrastructure: compiled with gcc -O2 -ffp-contract=off by tests/gram_ref.py; nothing of the product is
 * included or linked.  The rows X [n][K] come from the caller (phi from xview_ref.c, theta from the handle under test).
 *   y_r[k]      = X_r[k], or sqrt(X_r[k]) with transform == 1
 *   block b     = the rows [b * B, min((b + 1) * B, n)), B = 1024
 *   P_b[k][l]   = p after  p = +0.0; for r ascending in the block: p = fma(y_r[k], y_r[l], p)
 *   gram[k][l]  = g after  g = +0.0; for b ascending: g = g + P_b[k][l]
 *   sums[k]     = the same two levels with plain adds
 *   n_above[k]  = #{r : X_r[k] > threshold};  co_above[k][l] = #{r : X_r[k] > threshold and X_r[l] > threshold}
 * `variant` runs the sums in other ways, for the sensitivity tests alone: 1 = descending rows inside a block, 2 = unfused (p + a * b),
 * 3 = blocks of `block` rows instead of 1024, 4 = one chain over all rows, no blocks. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { GRAM_B = 1024 };

int gram_ref(int K, int64_t n, const double* x /*[n][K]*/, int transform, int variant, int64_t block, double* gram /*[K][K]*/, double* sums /*[K]*/)
{
    double* y = (double*)malloc((size_t)(n > 0 ? n : 1) * K * sizeof(double));
    if (!y) return -1;
    for (int64_t i = 0; i < n * K; i++) y[i] = transform ? sqrt(x[i]) : x[i];
    int64_t B = GRAM_B;
    if (variant == 3) B = block;
    if (variant == 4) B = n > 0 ? n : 1;
    for (int k = 0; k < K; k++) {
        for (int l = 0; l < K; l++) {
            double g = 0.0;
            for (int64_t b0 = 0; b0 < n; b0 += B) {
                const int64_t b1 = b0 + B < n ? b0 + B : n;
                double p = 0.0;
                if (variant == 1) for (int64_t r = b1 - 1; r >= b0; r--) p = fma(y[r * K + k], y[r * K + l], p);
                else if (variant == 2) for (int64_t r = b0; r < b1; r++) { const double t = y[r * K + k] * y[r * K + l]; p = p + t; }
                else for (int64_t r = b0; r < b1; r++) p = fma(y[r * K + k], y[r * K + l], p);
                g = g + p;
            }
            gram[(size_t)k * K + l] = g;
        }
        double s = 0.0;
        for (int64_t b0 = 0; b0 < n; b0 += B) {
            const int64_t b1 = b0 + B < n ? b0 + B : n;
            double q = 0.0;
            if (variant == 1) for (int64_t r = b1 - 1; r >= b0; r--) q = q + y[r * K + k];
            else for (int64_t r = b0; r < b1; r++) q = q + y[r * K + k];
            s = s + q;
        }
        sums[k] = s;
    }
    free(y);
    return 0;
}

void gram_counts(int K, int64_t n, const double* x /*[n][K]*/, double threshold, int64_t* n_above /*[K]*/, int64_t* co_above /*[K][K]*/)
{
    memset(n_above, 0, (size_t)K * sizeof(int64_t));
    memset(co_above, 0, (size_t)K * K * sizeof(int64_t));
    for (int64_t r = 0; r < n; r++)
        for (int k = 0; k < K; k++) {
            if (!(x[r * K + k] > threshold)) continue;
            n_above[k]++;
            for (int l = 0; l < K; l++)
                if (x[r * K + l] > threshold) co_above[(size_t)k * K + l]++;
        }
}
