/* ltr_ref.c -- TEST INFRASTRUCTURE: the left-to-right held-out estimator of include/mvhdp.h (mvhdp_heldout_left_to_right), restated
 * sequentially in plain C from the header's paragraphs: the model terms, the visit order, the summation order, the draw.  Nothing here is
 * taken from the kernel; the scan is written as the header describes it (four in-row steps, two row-total steps).
 * Compile without contraction (-ffp-contract=off, no -ffast-math): every operation is rounded on its own. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static void philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static double bits_to_unit(uint32_t hi, uint32_t lo)
{
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return (double)(x >> 11) * 0x1.0p-53;
}

/* the 64 lane sums scanned in the header's order */
static void lane_scan(double v[64])
{
    double o[64];
    for (int s = 1; s <= 8; s <<= 1) {
        memcpy(o, v, sizeof o);
        for (int l = 0; l < 64; l++)
            if ((l & 15) >= s) v[l] = o[l] + o[l - s];
    }
    memcpy(o, v, sizeof o);
    for (int l = 16; l < 32; l++) v[l] = o[l] + o[15];
    for (int l = 48; l < 64; l++) v[l] = o[l] + o[47];
    memcpy(o, v, sizeof o);
    for (int l = 32; l < 64; l++) v[l] = o[l] + o[31];
}

typedef struct {
    int K, V, T;
    const int32_t* nwk;                /* [V][K] */
    const double* alpha;               /* [K] */
    const double* rinv;                /* [K] */
    double beta, alpha_sum;
    uint32_t k0, k1;
} ltr_model;

/* the weights of token w under n_dk; returns the total, leaves wt [64 T], pre [64 T], excl [64] */
static double form_weights(const ltr_model* M, int w, const int32_t* ndk, double* wt, double* pre, double* excl)
{
    const int T = M->T, K = M->K;
    double s[64];
    for (int l = 0; l < 64; l++) {
        double run = 0.0;
        for (int j = 0; j < T; j++) {
            const int k = l * T + j;
            double x = 0.0;
            if (k < K) {
                const double phi = ((double)M->nwk[(size_t)w * K + k] + M->beta) * M->rinv[k];
                x = (M->alpha[k] + (double)ndk[k]) * phi;
            }
            wt[k] = x;
            run = j == 0 ? x : run + x;
            pre[k] = run;
        }
        s[l] = run;
    }
    lane_scan(s);
    excl[0] = 0.0;
    for (int l = 1; l < 64; l++) excl[l] = s[l - 1];
    return s[63];
}

static int draw(const ltr_model* M, const double* wt, const double* pre, const double* excl, double total, uint32_t c0, uint32_t c1, uint32_t limit, uint32_t position)
{
    const uint32_t ctr[4] = { c0, c1, limit, position };
    uint32_t x[4];
    philox4x32_10(ctr, M->k0, M->k1, x);
    const double target = bits_to_unit(x[0], x[1]) * total;
    int last = 0;
    for (int k = 0; k < 64 * M->T; k++) {
        if (!(wt[k] > 0.0)) continue;
        if (excl[k / M->T] + pre[k] > target) return k;
        last = k;
    }
    return last;
}

/* One call of the estimator on the host.  nk: [K] of the view; alpha: the K values used as alpha_k; alpha_sum: alphaSum'.
 * P (or NULL): [R][N] p_r[n].  Returns 0, or -1 on a bad argument. */
int ltr_evaluate(int K, int V, const int32_t* nwk, const int32_t* nk, double beta, const double* alpha, double alpha_sum,
                 int particles, int resample, uint64_t seed, int64_t doc_base, int64_t D, const int64_t* doc_off, const int32_t* tok,
                 double* S /*[N]*/, double* P, int64_t* doc_tokens /*[D]*/, int64_t* totals /*[3]: tokens, oov, visits*/)
{
    if (K < 1 || K > 2048 || particles < 1) return -1;
    ltr_model M;
    M.K = K; M.V = V; M.nwk = nwk; M.alpha = alpha; M.beta = beta; M.alpha_sum = alpha_sum;
    M.k0 = (uint32_t)seed; M.k1 = (uint32_t)(seed >> 32);
    M.T = 1;
    while (64 * M.T < K) M.T <<= 1;
    const int KT = 64 * M.T;
    const double beta_sum = beta * (double)V;
    double* rinv = (double*)malloc((size_t)K * sizeof(double));
    for (int k = 0; k < K; k++) rinv[k] = 1.0 / ((double)nk[k] + beta_sum);
    M.rinv = rinv;
    double* wt = (double*)malloc((size_t)KT * sizeof(double));
    double* pre = (double*)malloc((size_t)KT * sizeof(double));
    int32_t* ndk = (int32_t*)malloc((size_t)KT * sizeof(int32_t));
    double excl[64];
    const int64_t N = doc_off[D];
    for (int64_t i = 0; i < N; i++) S[i] = 0.0;
    totals[0] = totals[1] = totals[2] = 0;
    for (int64_t d = 0; d < D; d++) {
        const int64_t b = doc_off[d], L = doc_off[d + 1] - b;
        const uint64_t g = (uint64_t)(doc_base + d);
        int32_t* z = (int32_t*)malloc((size_t)(L > 0 ? L : 1) * sizeof(int32_t));
        int64_t in_vocab = 0;
        for (int64_t i = 0; i < L; i++) in_vocab += tok[b + i] < V;
        doc_tokens[d] = in_vocab;
        totals[0] += in_vocab; totals[1] += L - in_vocab;
        for (int r = 0; r < particles; r++) {
            const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)r + ((uint32_t)(g >> 32) << 20);
            memset(ndk, 0, (size_t)KT * sizeof(int32_t));
            int64_t tokens_so_far = 0;
            for (int64_t limit = 0; limit < L; limit++) {
                if (resample)
                    for (int64_t position = 0; position < limit; position++) {
                        const int w = tok[b + position];
                        if (w >= V) continue;
                        ndk[z[position]]--;
                        const double total = form_weights(&M, w, ndk, wt, pre, excl);
                        z[position] = draw(&M, wt, pre, excl, total, c0, c1, (uint32_t)limit, (uint32_t)position);
                        ndk[z[position]]++;
                        totals[2]++;
                    }
                const int w = tok[b + limit];
                if (w >= V) continue;
                const double total = form_weights(&M, w, ndk, wt, pre, excl);
                const double p = total / (alpha_sum + (double)tokens_so_far);
                if (P) P[(size_t)r * (size_t)N + (size_t)(b + limit)] = p;
                S[b + limit] = S[b + limit] + p;               /* r ascending */
                tokens_so_far++;
                z[limit] = draw(&M, wt, pre, excl, total, c0, c1, (uint32_t)limit, (uint32_t)limit);
                ndk[z[limit]]++;
                totals[2]++;
            }
        }
        free(z);
    }
    free(rinv); free(wt); free(pre); free(ndk);
    return 0;
}

void ltr_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { philox4x32_10(ctr, key[0], key[1], out); }
