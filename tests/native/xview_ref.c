/* xview_ref.c -- the sequential restatement of the cross-view prediction contract of include/mvhdp.h (mvhdp_predict_items,
 * mvhdp_score_items): plain loops, libm's fma, one entity and one type at a time.  Test infrastructure: compiled with
 * gcc -O2 -ffp-contract=off by tests/xview_ref.py; nothing of the product is included or linked.
 *   phi[w][k]   = ((double)n_wk[w][k] + beta) / ((double)n_k[k] + beta_sum), exactly 0.0 for an inactive topic
 *   score(d, w) = s after  s = +0.0; for k = 0 .. K-1: s = fma(theta[d][k], phi[w][k], s)
 *   order       = score descending, equal scores by ascending type id
 *   excluded(d) = the types < V in d's span (doc_off, tok), only with exclude_present
 * xview_chain's `variant` runs the chain in other ways, for the sensitivity tests alone: 1 = descending k, 2 = unfused (s + a * b). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

double xview_chain(int K, const double* theta, const double* phi, int variant)
{
    double s = 0.0;
    if (variant == 0) for (int k = 0; k < K; k++) s = fma(theta[k], phi[k], s);
    else if (variant == 1) for (int k = K - 1; k >= 0; k--) s = fma(theta[k], phi[k], s);
    else for (int k = 0; k < K; k++) { const double p = theta[k] * phi[k]; s = s + p; }
    return s;
}

void xview_phi(int K, int V, const int32_t* nwk, const int32_t* nk, const uint8_t* inactive, double beta, double beta_sum, double* phi /*[V][K]*/)
{
    for (int w = 0; w < V; w++)
        for (int k = 0; k < K; k++)
            phi[(size_t)w * K + k] = (inactive && inactive[k]) ? 0.0 : ((double)nwk[(size_t)w * K + k] + beta) / ((double)nk[k] + beta_sum);
}

/* scores[d][w] for every entity and type, by `variant` of the chain */
void xview_scores(int K, int V, int64_t D, const double* theta /*[D][K]*/, const double* phi /*[V][K]*/, int variant, double* scores /*[D][V]*/)
{
    for (int64_t d = 0; d < D; d++)
        for (int w = 0; w < V; w++) scores[(size_t)d * V + w] = xview_chain(K, theta + (size_t)d * K, phi + (size_t)w * K, variant);
}

/* a precedes b in the order */
static int precedes(double sa, int a, double sb, int b) { return sa > sb || (sa == sb && a < b); }

static void excluded_of(int V, int exclude_present, const int64_t* doc_off, const int32_t* tok, int64_t d, uint8_t* ex)
{
    memset(ex, 0, (size_t)V);
    if (!exclude_present) return;
    for (int64_t i = doc_off[d]; i < doc_off[d + 1]; i++)
        if (tok[i] >= 0 && tok[i] < V) ex[tok[i]] = 1;
}

/* the first min(n, V - |excluded|) types of every entity by selection, one at a time; unused slots: item -1, score 0.0 */
int xview_predict(int V, int64_t D, const double* scores /*[D][V]*/, int exclude_present, const int64_t* doc_off, const int32_t* tok, int n,
                  int32_t* items /*[D][n]*/, double* out_scores /*[D][n]*/, int32_t* counts /*[D]*/)
{
    uint8_t* ex = (uint8_t*)malloc((size_t)V);
    uint8_t* taken = (uint8_t*)malloc((size_t)V);
    if (!ex || !taken) return -1;
    for (int64_t d = 0; d < D; d++) {
        const double* s = scores + (size_t)d * V;
        excluded_of(V, exclude_present, doc_off, tok, d, ex);
        memset(taken, 0, (size_t)V);
        int c = 0;
        for (; c < n; c++) {
            int best = -1;
            for (int w = 0; w < V; w++) {
                if (ex[w] || taken[w]) continue;
                if (best < 0 || precedes(s[w], w, s[best], best)) best = w;
            }
            if (best < 0) break;
            taken[best] = 1;
            items[(size_t)d * n + c] = best;
            out_scores[(size_t)d * n + c] = s[best];
        }
        counts[d] = c;
        for (; c < n; c++) { items[(size_t)d * n + c] = -1; out_scores[(size_t)d * n + c] = 0.0; }
    }
    free(ex); free(taken);
    return 0;
}

/* per pair: the score, and the number of types w' != item that are not excluded for the entity and precede item */
int xview_score_pairs(int V, const double* scores /*[D][V]*/, int exclude_present, const int64_t* doc_off, const int32_t* tok, int64_t n_pairs,
                      const int64_t* entity, const int32_t* item, double* score, int32_t* rank)
{
    uint8_t* ex = (uint8_t*)malloc((size_t)V);
    if (!ex) return -1;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t d = entity[p];
        const int q = item[p];
        const double* s = scores + (size_t)d * V;
        excluded_of(V, exclude_present, doc_off, tok, d, ex);
        int32_t r = 0;
        for (int w = 0; w < V; w++)
            if (w != q && !ex[w] && precedes(s[w], w, s[q], q)) r++;
        score[p] = s[q];
        rank[p] = r;
    }
    free(ex);
    return 0;
}
