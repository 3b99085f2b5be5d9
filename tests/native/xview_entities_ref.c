/* xview_entities_ref.c -- the sequential restatement of the entities-for-an-item contract of include/mvhdp.h (mvhdp_predict_entities,
 * mvhdp_rank_entities): plain loops, libm's fma, one query and one entity at a time.  Test infrastructure: compiled with
 * gcc -O2 -ffp-contract=off by tests/xview_entities_ref.py, together with xview_ref.c whose xview_phi makes the phi table; nothing of
 * the product is included or linked.  Inputs: theta rows [C][K] of the candidates and the count table.
 *   psi[j][k]    = p after  p = +0.0; for the query's items i ascending: p = fma(c_i, phi[w_i][k], p)       (c_i = 1.0 without weights)
 *   score(d, j)  = s after  s = +0.0; for k = 0 .. K-1: s = fma(theta[d][k], psi[j][k], s)
 *   order        = score descending, equal scores by ascending entity
 *   excluded(j)  = the entities whose span (doc_off, tok) holds an item of query j, only with exclude_present */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void xview_phi(int K, int V, const int32_t* nwk, const int32_t* nk, const uint8_t* inactive, double beta, double beta_sum, double* phi);

/* phi [V][K] by xview_ref.c from the counts, then the query rows */
int xve_psi_from_counts(int K, int V, const int32_t* nwk, const int32_t* nk, const uint8_t* inactive, double beta, double beta_sum, int64_t nq,
                        const int64_t* q_off, const int32_t* q_items, const double* q_weights /* or NULL */, double* psi /*[nq][K]*/)
{
    double* phi = (double*)malloc((size_t)V * K * sizeof(double));
    if (!phi) return -1;
    xview_phi(K, V, nwk, nk, inactive, beta, beta_sum, phi);
    for (int64_t j = 0; j < nq; j++)
        for (int k = 0; k < K; k++) {
            double p = 0.0;
            for (int64_t i = q_off[j]; i < q_off[j + 1]; i++) p = fma(q_weights ? q_weights[i] : 1.0, phi[(size_t)q_items[i] * K + k], p);
            psi[(size_t)j * K + k] = p;
        }
    free(phi);
    return 0;
}

/* scores[j][d] for every query and candidate */
void xve_scores(int K, int64_t nq, int64_t C, const double* theta /*[C][K]*/, const double* psi /*[nq][K]*/, double* scores /*[nq][C]*/)
{
    for (int64_t j = 0; j < nq; j++)
        for (int64_t d = 0; d < C; d++) {
            double s = 0.0;
            for (int k = 0; k < K; k++) s = fma(theta[(size_t)d * K + k], psi[(size_t)j * K + k], s);
            scores[(size_t)j * C + d] = s;
        }
}

/* ex[j][d] = 1 when candidate d's span holds an item of query j; doc_off / tok: the spans of the candidates alone */
void xve_excluded(int64_t C, const int64_t* doc_off /*[C+1]*/, const int32_t* tok, int64_t nq, const int64_t* q_off, const int32_t* q_items, uint8_t* ex /*[nq][C]*/)
{
    memset(ex, 0, (size_t)nq * (size_t)C);
    for (int64_t j = 0; j < nq; j++)
        for (int64_t d = 0; d < C; d++)
            for (int64_t t = doc_off[d]; t < doc_off[d + 1] && !ex[(size_t)j * C + d]; t++)
                for (int64_t i = q_off[j]; i < q_off[j + 1]; i++)
                    if (q_items[i] == tok[t]) { ex[(size_t)j * C + d] = 1; break; }
}

/* a precedes b in the order */
static int precedes(double sa, int64_t a, double sb, int64_t b) { return sa > sb || (sa == sb && a < b); }

/* per query the first min(n, candidates not excluded) by selection, one at a time; ids = id0 + candidate; unused slots: id -1, score 0.0 */
int xve_predict(int64_t nq, int64_t C, const double* scores /*[nq][C]*/, const uint8_t* ex /*[nq][C] or NULL*/, int n, int64_t id0,
                int64_t* ids /*[nq][n]*/, double* out_scores /*[nq][n]*/, int32_t* counts /*[nq]*/)
{
    uint8_t* taken = (uint8_t*)malloc((size_t)(C > 0 ? C : 1));
    if (!taken) return -1;
    for (int64_t j = 0; j < nq; j++) {
        const double* s = scores + (size_t)j * C;
        memset(taken, 0, (size_t)C);
        int c = 0;
        for (; c < n; c++) {
            int64_t best = -1;
            for (int64_t d = 0; d < C; d++) {
                if ((ex && ex[(size_t)j * C + d]) || taken[d]) continue;
                if (best < 0 || precedes(s[d], d, s[best], best)) best = d;
            }
            if (best < 0) break;
            taken[best] = 1;
            ids[(size_t)j * n + c] = id0 + best;
            out_scores[(size_t)j * n + c] = s[best];
        }
        counts[j] = c;
        for (; c < n; c++) { ids[(size_t)j * n + c] = -1; out_scores[(size_t)j * n + c] = 0.0; }
    }
    free(taken);
    return 0;
}

/* per pair (query, candidate): the score, and the number of candidates d' != candidate that are not excluded for the query and precede it */
void xve_rank(int64_t C, const double* scores /*[nq][C]*/, const uint8_t* ex /*[nq][C] or NULL*/, int64_t n_pairs, const int64_t* query,
              const int64_t* cand, double* score, int64_t* rank)
{
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t j = query[p], q = cand[p];
        const double* s = scores + (size_t)j * C;
        int64_t r = 0;
        for (int64_t d = 0; d < C; d++)
            if (d != q && !(ex && ex[(size_t)j * C + d]) && precedes(s[d], d, s[q], q)) r++;
        score[p] = s[q];
        rank[p] = r;
    }
}
