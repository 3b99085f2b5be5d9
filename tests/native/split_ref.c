/* split_ref.c -- the sequential restatement of mvhdp_split_topic as include/mvhdp.h defines it: the split set, the target, the constants of
 * the call, the initial sides, the frozen word counts per iteration, the live side counts of an entity, the visit.  Nothing here is taken
 * from the kernel.  Philox and bits_to_unit are the functions of foldin_ref.c, copied.
 * Compile without contraction (-ffp-contract=off, no -ffast-math): every operation is rounded on its own. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAXM 8
#define KEEP_ALPHA 0x1u
enum { OK = 0, ERR_INVALID_ARG = -1 };

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

static double unit_of(uint64_t g, uint32_t it, int m, uint32_t pos, uint64_t seed)
{
    const uint32_t ctr[4] = { (uint32_t)g, (uint32_t)(g >> 32), it + ((uint32_t)m << 16), pos };
    uint32_t x[4];
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    return bits_to_unit(x[0], x[1]);
}

/* z [M] -> [N_m] is rewritten in place; alpha [M][K + 1] and inactive [K] likewise.  nk [M][K] is read only (the target's condition).
 * P [M][M] is the coupling already resolved (the default is the wrapper's).  hint [M] -> NULL or [V_m].  stats: split [8], moved [8],
 * flips_last, target, activated as int64 [19].  flips [iterations] or NULL.  trace: NULL, or [trace_cap][4] of (u, wt[a], wt[b], total)
 * in visit order (entity, view, position within an iteration), *n_trace visits written.
 * Returns OK or ERR_INVALID_ARG for the refusals that belong to the arguments and the model (the handle's state is not this file's). */
int split_run(int K, int M, const int32_t* V, int64_t D, const int64_t* const* doc_off, const int32_t* const* tokens, int32_t* const* z,
              const int32_t* nk, const double* beta, const double* beta_sum, const double* gamma, double* alpha, const double* alpha_sum,
              uint8_t* inactive, const double* P, int32_t source, int32_t target, int32_t iterations, uint32_t flags, uint64_t seed,
              int64_t doc_id_base, const int8_t* const* hint, int64_t* stats, int64_t* flips, double* trace, int64_t trace_cap, int64_t* n_trace)
{
    if (flags & ~KEEP_ALPHA) return ERR_INVALID_ARG;
    if (iterations < 0 || iterations > 65535) return ERR_INVALID_ARG;
    if (source < 0 || source >= K || target < -1 || target >= K || source == target) return ERR_INVALID_ARG;
    if (inactive[source]) return ERR_INVALID_ARG;
    for (int i = 0; i < M * M; i++)
        if (!(P[i] >= 0.0) || !isfinite(P[i])) return ERR_INVALID_ARG;
    if (hint)
        for (int m = 0; m < M; m++)
            if (hint[m])
                for (int w = 0; w < V[m]; w++)
                    if (hint[m][w] < -1 || hint[m][w] > 1) return ERR_INVALID_ARG;
    /* the target */
    if (target < 0) {
        for (int t = 0; t < K && target < 0; t++) {
            if (t == source || !inactive[t]) continue;
            int is_free = 1;
            for (int m = 0; m < M; m++) is_free = is_free && nk[(size_t)m * K + t] == 0 && alpha[(size_t)m * (K + 1) + t] == 0.0;
            if (is_free) target = t;
        }
        if (target < 0) return ERR_INVALID_ARG;
    } else {
        for (int m = 0; m < M; m++)
            if (nk[(size_t)m * K + target] != 0 || alpha[(size_t)m * (K + 1) + target] != 0.0) return ERR_INVALID_ARG;
    }

    /* the constants of the call */
    double ah[MAXM], A[MAXM], gas[MAXM];
    for (int m = 0; m < M; m++) {
        ah[m] = 0.5 * alpha[(size_t)m * (K + 1) + source];
        A[m] = gamma[m] * ah[m];
        gas[m] = gamma[m] * alpha_sum[m];
    }

    /* the sides: per view one byte per position, meaningful where z == source */
    uint8_t* side[MAXM];
    int32_t* cw[MAXM];                                         /* [V_m][2], frozen */
    int32_t* cw_next[MAXM];                                    /* the counts the iteration leaves */
    int64_t c[MAXM][2], c_next[MAXM][2];
    for (int m = 0; m < M; m++) {
        const int64_t N = doc_off[m][D];
        side[m] = (uint8_t*)calloc((size_t)(N > 0 ? N : 1), 1);
        cw[m] = (int32_t*)calloc((size_t)V[m] * 2, sizeof(int32_t));
        cw_next[m] = (int32_t*)calloc((size_t)V[m] * 2, sizeof(int32_t));
        c[m][0] = c[m][1] = 0;
        stats[m] = 0;
    }

    /* iteration 0 */
    for (int64_t d = 0; d < D; d++)
        for (int m = 0; m < M; m++)
            for (int64_t n = doc_off[m][d]; n < doc_off[m][d + 1]; n++) {
                if (z[m][n] != source) continue;
                const int32_t w = tokens[m][n];
                const int hv = (hint && hint[m]) ? hint[m][w] : -1;
                int s;
                if (hv == 0 || hv == 1) s = hv;
                else s = unit_of((uint64_t)(doc_id_base + d), 0u, m, (uint32_t)(n - doc_off[m][d]), seed) >= 0.5 ? 1 : 0;
                side[m][n] = (uint8_t)s;
                cw[m][2 * (size_t)w + s]++;
                c[m][s]++;
                stats[m]++;
            }

    int64_t nt = 0;
    for (int it = 1; it <= iterations; it++) {
        for (int m = 0; m < M; m++) {
            memcpy(cw_next[m], cw[m], (size_t)V[m] * 2 * sizeof(int32_t));
            c_next[m][0] = c[m][0]; c_next[m][1] = c[m][1];
        }
        int64_t nflips = 0;
        for (int64_t d = 0; d < D; d++) {
            int64_t e[MAXM][2];
            for (int m = 0; m < M; m++) {
                e[m][0] = e[m][1] = 0;
                for (int64_t n = doc_off[m][d]; n < doc_off[m][d + 1]; n++)
                    if (z[m][n] == source) e[m][side[m][n]]++;
            }
            for (int m = 0; m < M; m++) {
                const int64_t len_m = doc_off[m][d + 1] - doc_off[m][d];
                if (e[m][0] + e[m][1] == 0) continue;
                const double Lp_m = (double)len_m + gas[m];
                double base[2], r0[2], r1[2];
                for (int x = 0; x < 2; x++) {
                    double s = 0.0;
                    for (int i = 0; i < M; i++) {
                        if (i == m) continue;
                        const int64_t len_i = doc_off[i][d + 1] - doc_off[i][d];
                        if (len_i == 0) continue;
                        const double Lp_i = (double)len_i + gas[i];
                        s = s + P[m * M + i] * ((double)e[i][x] + A[i]) / Lp_i;
                    }
                    base[x] = A[m] + s * Lp_m;
                    r0[x] = 1.0 / ((double)c[m][x] + beta_sum[m]);
                    r1[x] = 1.0 / ((double)(c[m][x] - 1) + beta_sum[m]);
                }
                for (int64_t n = doc_off[m][d]; n < doc_off[m][d + 1]; n++) {
                    if (z[m][n] != source) continue;
                    const int32_t w = tokens[m][n];
                    const int y = side[m][n];
                    e[m][y]--;
                    double wt[2];
                    for (int x = 0; x < 2; x++) {
                        const int own = x == y;
                        const double phi = ((double)(cw[m][2 * (size_t)w + x] - own) + beta[m]) * (own ? r1[x] : r0[x]);
                        wt[x] = (P[m * M + m] * (double)e[m][x] + base[x]) * phi;
                    }
                    const double total = wt[0] + wt[1];
                    const double u = unit_of((uint64_t)(doc_id_base + d), (uint32_t)it, m, (uint32_t)(n - doc_off[m][d]), seed);
                    int s = u * total < wt[0] ? 0 : 1;
                    if (total == 0.0 || !isfinite(total)) s = y;
                    if (trace && nt < trace_cap) { double* t = trace + 4 * nt; t[0] = u; t[1] = wt[0]; t[2] = wt[1]; t[3] = total; }
                    nt++;
                    e[m][s]++;
                    if (s != y) {
                        side[m][n] = (uint8_t)s;
                        cw_next[m][2 * (size_t)w + y]--; cw_next[m][2 * (size_t)w + s]++;
                        c_next[m][y]--; c_next[m][s]++;
                        nflips++;
                    }
                }
            }
        }
        for (int m = 0; m < M; m++) {
            int32_t* t = cw[m]; cw[m] = cw_next[m]; cw_next[m] = t;
            c[m][0] = c_next[m][0]; c[m][1] = c_next[m][1];
        }
        if (flips) flips[it - 1] = nflips;
        stats[2 * MAXM] = nflips;
    }
    if (iterations == 0) stats[2 * MAXM] = 0;
    if (n_trace) *n_trace = nt < trace_cap ? nt : trace_cap;

    /* afterwards */
    for (int m = 0; m < M; m++) {
        const int64_t N = doc_off[m][D];
        int64_t moved = 0;
        for (int64_t n = 0; n < N; n++)
            if (z[m][n] == source && side[m][n]) { z[m][n] = target; moved++; }
        stats[MAXM + m] = moved;
        if (!(flags & KEEP_ALPHA)) alpha[(size_t)m * (K + 1) + source] = ah[m];
        alpha[(size_t)m * (K + 1) + target] = ah[m];
        free(side[m]); free(cw[m]); free(cw_next[m]);
    }
    stats[2 * MAXM + 1] = target;
    stats[2 * MAXM + 2] = inactive[target] ? 1 : 0;
    inactive[target] = 0;
    return OK;
}

void split_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { philox4x32_10(ctr, key[0], key[1], out); }
double split_unit(uint32_t hi, uint32_t lo) { return bits_to_unit(hi, lo); }
