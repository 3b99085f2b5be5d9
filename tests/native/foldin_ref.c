/* foldin_ref.c -- TEST INFRASTRUCTURE: the fold-in of include/mvhdp.h (mvhdp_fold_in), restated sequentially in plain C from the header's
 * paragraphs: the weights, the coupling, one iteration, the draw (with the summation order of the held-out paragraph it refers to), the
 * samples, theta.  Nothing here is taken from the kernel.  Philox, bits_to_unit and the lane scan are the functions of ltr_ref.c, copied.
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

/* One call on the host.  nwk[m]: [V_m][K]; nk, alpha: [M][K]; P: [M][M]; w: [M] or NULL (no theta); doc_off[m] (or NULL) / tok[m] per view;
 * z[m] (or NULL): [N_m]; counts_sum: [D][M][K]; totals: tokens, oov, visits.  trace_wt (or NULL; one document): per visit in order
 * total, u, wt[0..K);  trace_base (or NULL; one document): [iterations][M][K] base_m of every pass (0 where the view has no pass).
 * Returns 0, or -1 on a bad argument. */
int foldin_run(int K, int M, const int32_t* V, const int32_t* const* nwk, const int32_t* nk, const double* beta, const double* beta_sum,
               const double* gamma, const double* alpha, const double* alpha_sum, const uint8_t* inactive, const double* P,
               int iterations, int S, int thin, uint64_t seed, int64_t doc_base, int64_t D, const int64_t* const* doc_off, const int32_t* const* tok,
               const double* w, double* theta, int32_t* const* z, int32_t* counts_sum, int64_t* totals, double* trace_wt, double* trace_base)
{
    if (K < 1 || K > 2048 || M < 1 || M > 8 || iterations < 1 || iterations > 65535 || S < 1 || thin < 1 || iterations - (S - 1) * thin < 1 || doc_base < 0) return -1;
    if ((trace_wt || trace_base) && D != 1) return -1;
    int T = 1;
    while (64 * T < K) T <<= 1;
    const int KT = 64 * T;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double* a = (double*)calloc((size_t)M * K, sizeof(double));
    double* rinv = (double*)calloc((size_t)M * K, sizeof(double));
    for (int m = 0; m < M; m++)
        for (int k = 0; k < K; k++) {
            a[m * K + k] = gamma[m] * alpha[m * K + k];
            rinv[m * K + k] = 1.0 / ((double)nk[m * K + k] + beta_sum[m]);
        }
    int32_t* ndk = (int32_t*)malloc((size_t)M * K * sizeof(int32_t));
    double* base = (double*)malloc((size_t)K * sizeof(double));
    double* wt = (double*)malloc((size_t)KT * sizeof(double));
    double* pre = (double*)malloc((size_t)KT * sizeof(double));
    totals[0] = totals[1] = totals[2] = 0;
    int64_t n_trace = 0;
    for (int64_t d = 0; d < D; d++) {
        const uint64_t g = (uint64_t)(doc_base + d);
        int64_t len[8], b[8];
        int32_t* zz[8];
        for (int m = 0; m < M; m++) {
            b[m] = doc_off[m] ? doc_off[m][d] : 0;
            len[m] = doc_off[m] ? doc_off[m][d + 1] - b[m] : 0;
            zz[m] = (int32_t*)malloc((size_t)(len[m] > 0 ? len[m] : 1) * sizeof(int32_t));
            for (int64_t i = 0; i < len[m]; i++) {
                zz[m][i] = -1;
                if (tok[m][b[m] + i] < V[m]) totals[0]++; else totals[1]++;
            }
        }
        memset(ndk, 0, (size_t)M * K * sizeof(int32_t));
        int32_t* cs = counts_sum + (size_t)d * M * K;
        memset(cs, 0, (size_t)M * K * sizeof(int32_t));
        for (int it = 1; it <= iterations; it++) {
            for (int m = 0; m < M; m++) {
                if (len[m] == 0) continue;
                const double Lp_m = (double)len[m] + gamma[m] * alpha_sum[m];
                for (int k = 0; k < K; k++) {
                    double s = 0.0;
                    for (int i = 0; i < M; i++) {
                        if (i == m || len[i] == 0) continue;
                        const double Lp_i = (double)len[i] + gamma[i] * alpha_sum[i];
                        s = s + P[m * M + i] * ((double)ndk[i * K + k] + a[i * K + k]) / Lp_i;
                    }
                    const double o = s * Lp_m;
                    base[k] = a[m * K + k] + o;
                    if (trace_base) trace_base[((size_t)(it - 1) * M + m) * K + k] = base[k];
                }
                for (int64_t pos = 0; pos < len[m]; pos++) {
                    const int32_t wd = tok[m][b[m] + pos];
                    if (wd >= V[m]) continue;
                    const int old = zz[m][pos];
                    if (old >= 0) ndk[m * K + old]--;
                    /* the weights, the in-lane prefix sums, the scan */
                    double sl[64], excl[64];
                    for (int l = 0; l < 64; l++) {
                        double run = 0.0;
                        for (int j = 0; j < T; j++) {
                            const int k = l * T + j;
                            double x = 0.0;
                            if (k < K) {
                                double phi = ((double)nwk[m][(size_t)wd * K + k] + beta[m]) * rinv[m * K + k];
                                if (inactive && inactive[k]) phi = 0.0;
                                x = (P[m * M + m] * (double)ndk[m * K + k] + base[k]) * phi;
                            }
                            wt[k] = x;
                            run = j == 0 ? x : run + x;
                            pre[k] = run;
                        }
                        sl[l] = run;
                    }
                    lane_scan(sl);
                    excl[0] = 0.0;
                    for (int l = 1; l < 64; l++) excl[l] = sl[l - 1];
                    const double total = sl[63];
                    totals[2]++;
                    const uint32_t ctr[4] = { (uint32_t)g, (uint32_t)(g >> 32), (uint32_t)it + ((uint32_t)m << 16), (uint32_t)pos };
                    uint32_t x[4];
                    philox4x32_10(ctr, k0, k1, x);
                    const double u = bits_to_unit(x[0], x[1]);
                    if (trace_wt) {
                        double* t = trace_wt + (size_t)n_trace * (K + 2);
                        t[0] = total; t[1] = u;
                        memcpy(t + 2, wt, (size_t)K * sizeof(double));
                        n_trace++;
                    }
                    int zn = old;
                    if (total != 0.0 && isfinite(total)) {
                        const double target = u * total;
                        int last = -1, found = -1;
                        for (int k = 0; k < KT && found < 0; k++) {
                            if (!(wt[k] > 0.0)) continue;
                            if (excl[k / T] + pre[k] > target) found = k;
                            last = k;
                        }
                        zn = found >= 0 ? found : last;
                    }
                    zz[m][pos] = zn;
                    if (zn >= 0) ndk[m * K + zn]++;
                }
            }
            const int back = iterations - it;
            if (back % thin == 0 && back / thin <= S - 1)
                for (int i = 0; i < M * K; i++) cs[i] += ndk[i];
        }
        if (theta && w) {
            double norm = 0;
            for (int m = 0; m < M; m++) norm += w[m];
            for (int k = 0; k < K; k++) {
                double tp = 0;
                for (int m = 0; m < M; m++)
                    tp += w[m] * ((double)cs[m * K + k] / (double)S + gamma[m] * alpha[m * K + k]) / ((double)len[m] + gamma[m] * alpha_sum[m]);
                theta[(size_t)d * K + k] = tp / norm;
            }
        }
        for (int m = 0; m < M; m++) {
            if (z && z[m]) memcpy(z[m] + b[m], zz[m], (size_t)len[m] * sizeof(int32_t));
            free(zz[m]);
        }
    }
    free(a); free(rinv); free(ndk); free(base); free(wt); free(pre);
    return 0;
}

void foldin_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { philox4x32_10(ctr, key[0], key[1], out); }
double foldin_unit(uint32_t hi, uint32_t lo) { return bits_to_unit(hi, lo); }
