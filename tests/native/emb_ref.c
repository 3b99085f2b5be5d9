/*
 * emb_ref.c -- TEST INFRASTRUCTURE, never shipped: a sequential restatement of TopicWordEmbeddings + TopicWordEmbeddingRunnable
 * (TWE:126-163, 341-401; TWER:82-293) and of CalcSoftmaxTopicWordProbabilities (PTM:337-367) under the device's contract
 * (mvtopicmodel_amd/csrc/mvhdp_emb.hip): the same Philox draws, and every dot product of the trainer in the wave's
 * order (lane l sums its columns l, l + 64, l + 128, l + 192 from 0.0, then the butterfly over lanes 32, 16, .., 1).  This is what
 * the serial device flavour must equal bit for bit.  tests/emb_ref.py builds it with gcc -O2 -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void er_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out)
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

uint64_t er_draw64(uint32_t n, uint32_t purpose, uint32_t ent, uint32_t epoch, uint32_t k0, uint32_t k1)
{
    const uint32_t c[4] = {n >> 1, purpose, ent, epoch}, k[2] = {k0, k1};
    uint32_t x[4];
    er_philox(c, k, x);
    return (n & 1u) ? ((uint64_t)x[2] << 32 | x[3]) : ((uint64_t)x[0] << 32 | x[1]);
}

static double unit(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }
static uint64_t mulhi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

/* sigmoidCache TWE:157-162: cache[size] is never set */
void er_cache(int size, double min_exp, double max_exp, double* cache)
{
    for (int i = 0; i < size; i++) {
        const double value = ((double)i / size) * (max_exp - min_exp) + min_exp;
        cache[i] = 1.0 / (1.0 + exp(-value));
    }
    cache[size] = 0.0;
}

/* TWE:143-148 under the 0x503 stream */
void er_init(int64_t R, int C, uint64_t seed, double* w, double* neg)
{
    for (int64_t r = 0; r < R; r++)
        for (int c = 0; c < C; c++) {
            w[r * C + c] = (unit(er_draw64((uint32_t)c, 0x503u, (uint32_t)r, 0u, (uint32_t)seed, (uint32_t)(seed >> 32))) - 0.5) / (double)C;
            neg[r * C + c] = 0.0;
        }
}

/* countWords TWE:341-401: counts and total are cumulative (in and out); retention, the IDSorter order, the count^0.75 prefix sums */
static const int64_t* g_cnt;
static int by_count(const void* a, const void* b)
{
    const int32_t x = *(const int32_t*)a, y = *(const int32_t*)b;
    if (g_cnt[x] != g_cnt[y]) return g_cnt[x] > g_cnt[y] ? -1 : 1;
    return x > y ? -1 : (x < y);
}
void er_count(int V0, int64_t N, const int32_t* tok, double f, int64_t* counts, int64_t* total, double* retention, int32_t* sorted, double* dist)
{
    for (int64_t i = 0; i < N; i++) counts[tok[i]]++;
    *total += N;
    for (int w = 0; w < V0; w++) {
        const double s = (double)counts[w] / (f * (double)*total);
        const double r = (sqrt(s) + 1) / s;
        retention[w] = r < 1.0 ? r : 1.0;
    }
    for (int w = 0; w < V0; w++) sorted[w] = w;
    g_cnt = counts;
    qsort(sorted, (size_t)V0, sizeof(int32_t), by_count);
    dist[0] = pow((double)counts[sorted[0]], 0.75);
    for (int w = 1; w < V0; w++) dist[w] = dist[w - 1] + pow((double)counts[sorted[w]], 0.75);
}

/* the table as the device builds it: one lower_bound per index */
void er_table(int V0, const int32_t* sorted, const double* dist, int64_t size, int64_t first, int64_t n, int32_t* out)
{
    const double S = dist[V0 - 1];
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = first + j;
        int o = 0;
        if (i > 0) {
            const double x = S * (double)(i - 1) / (double)size;
            int lo = 0, hi = V0 - 1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (dist[mid] >= x) hi = mid; else lo = mid + 1; }
            o = lo;
        }
        out[j] = sorted[o];
    }
}

/* the table as TWE:393-399 writes it */
void er_table_literal(int V0, const int32_t* sorted, const double* dist, int64_t size, int32_t* out)
{
    const double samplingSum = dist[V0 - 1];
    int order = 0;
    for (int64_t i = 0; i < size; i++) {
        out[i] = sorted[order];
        while (samplingSum * i / size > dist[order] && order < V0 - 1) order++;
    }
}

typedef struct {
    const int64_t* doc_off; const int32_t* tok; const int32_t* z;       /* z NULL: no topics */
    int64_t D, N0, total_words, ent_base;
    int32_t V0, C, Cc, window, ns, min_len, epochs, cache_size;
    int64_t table_size; const int32_t* table; const double* retention; const double* cache;
    double min_exp, max_exp;
    uint64_t seed; uint32_t round, reserved;
} ErTrain;

typedef struct { int64_t words, sampled, considered, skipped, calls, negskip; double residual, last_residual; int64_t last_calls; } ErStats;

typedef struct {
    const ErTrain* a; double* w; double* neg;
    uint32_t ent, epoch, call, k0, k1;
    double lr, res, scale;
    int64_t calls, negskip;
} St;

static double wave_dot(const double* x, const double* y, int lo, int hi)
{
    double p[64], t[64];
    for (int l = 0; l < 64; l++) {
        double s = 0.0;
        for (int j = 0; j < 4; j++) {
            const int c = l + 64 * j, act = c >= lo && c < hi;
            s += (act ? x[c] : 0.0) * (act ? y[c] : 0.0);
        }
        p[l] = s;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        for (int l = 0; l < 64; l++) t[l] = p[l] + p[l ^ o];
        memcpy(p, t, sizeof p);
    }
    return p[0];
}

double er_residual(double dot, double lr, int positive, const double* cache, int cache_size, double min_exp, double max_exp)
{
    const double scale = (double)cache_size / (max_exp - min_exp);
    if (dot < min_exp) return positive ? lr : 0.0;
    if (dot > max_exp) return positive ? 0.0 : -lr;
    const double c = cache[(int)floor((dot - min_exp) * scale)];
    return positive ? lr * (1.0 - c) : lr * -c;
}

/* gradientLearn TWER:82-152 */
static void learn(St* s, int in, int out, int ctx)
{
    const ErTrain* a = s->a;
    const int C = a->C, lo = ctx ? 0 : a->Cc, hi = ctx ? a->Cc : C, ns = a->ns;
    double* ni = s->neg + (int64_t)in * C;
    double* wo = s->w + (int64_t)out * C;
    double grad[256];
    const double inv = 1.0 / ns;
    double g = er_residual(wave_dot(ni, wo, lo, hi), s->lr, 1, a->cache, a->cache_size, a->min_exp, a->max_exp);
    for (int c = lo; c < hi; c++) { grad[c] = g * ni[c]; ni[c] += g * wo[c]; }
    s->res += g;
    for (int q = 0; q < ns; q++) {
        const uint64_t x = er_draw64(s->call * (uint32_t)ns + (uint32_t)q, 0x502u, s->ent, s->epoch, s->k0, s->k1);
        const int t = a->table[mulhi(x, (uint64_t)a->table_size)];
        if (t == in) { s->negskip++; continue; }
        double* nt = s->neg + (int64_t)t * C;
        g = er_residual(wave_dot(nt, wo, lo, hi), s->lr, 0, a->cache, a->cache_size, a->min_exp, a->max_exp);
        for (int c = lo; c < hi; c++) { grad[c] += g * nt[c]; nt[c] += g * wo[c]; }
        s->res -= g * inv;
    }
    s->call++;
    s->calls++;
    for (int c = lo; c < hi; c++) wo[c] += grad[c];
}

/* TWER:155-293, every entity in id order, epochs in order (the serial device flavour) */
int er_train(const ErTrain* a, double* w, double* neg, ErStats* st)
{
    memset(st, 0, sizeof *st);
    St s;
    memset(&s, 0, sizeof s);
    s.a = a; s.w = w; s.neg = neg;
    s.k0 = (uint32_t)a->seed ^ a->round; s.k1 = (uint32_t)(a->seed >> 32);
    const double lr_min = 0.025 * 0.0001;
    const double denom = (double)((int64_t)a->epochs * a->total_words);
    int64_t maxlen = 1;
    for (int64_t d = 0; d < a->D; d++) if (a->doc_off[d + 1] - a->doc_off[d] > maxlen) maxlen = a->doc_off[d + 1] - a->doc_off[d];
    int32_t* buf = malloc((size_t)maxlen * sizeof(int32_t));
    int32_t* top = malloc((size_t)maxlen * sizeof(int32_t));
    if (!buf || !top) { free(buf); free(top); return -1; }
    int64_t prev_calls = 0;
    for (int ep = 0; ep < a->epochs; ep++) {
        s.epoch = (uint32_t)ep;
        s.res = 0.0;
        for (int64_t d = 0; d < a->D; d++) {
            const int64_t b = a->doc_off[d];
            const int L = (int)(a->doc_off[d + 1] - b);
            s.ent = (uint32_t)(a->ent_base + d);
            s.call = 0;
            s.lr = fmax(lr_min, 0.025 * (1.0 - (double)((int64_t)ep * a->N0 + b) / denom));
            int len = 0;
            for (int p = 0; p < L; p++) {
                const int ty = a->tok[b + p];
                if (unit(er_draw64((uint32_t)p, 0x500u, s.ent, s.epoch, s.k0, s.k1)) < a->retention[ty]) {
                    buf[len] = ty;
                    top[len] = a->z ? a->z[b + p] : 0;
                    len++;
                }
            }
            st->words += L; st->sampled += len;
            if (len < a->min_len) { st->skipped++; continue; }
            st->considered += len;
            for (int p = 0; p < len; p++) {
                const int in = buf[p], ta = a->V0 + top[p];
                if (a->z) { learn(&s, in, ta, 1); learn(&s, in, ta, 0); learn(&s, ta, in, 0); }
                const int sw = (int)mulhi(er_draw64((uint32_t)p, 0x501u, s.ent, s.epoch, s.k0, s.k1), (uint64_t)a->window) + 1;
                const int q0 = p - sw > 0 ? p - sw : 0, q1 = p + sw < len - 1 ? p + sw : len - 1;
                for (int q = q0; q <= q1; q++) {
                    if (q == p) continue;
                    learn(&s, in, buf[q], 0);
                    if (a->z) learn(&s, ta, a->V0 + top[q], 1);
                }
            }
        }
        st->residual += s.res;
        st->last_residual = s.res;
        st->last_calls = s.calls - prev_calls;
        prev_calls = s.calls;
    }
    st->calls = s.calls;
    st->negskip = s.negskip;
    free(buf); free(top);
    return 0;
}

/* CalcSoftmaxTopicWordProbabilities PTM:337-367: expdot [K][V0]; sums [K] accumulated (never reset, PTM:360) */
void er_softmax(int V0, int K, int C, const double* w, double* expdot, double* sums)
{
    for (int t = 0; t < K; t++) {
        const double* y = w + (int64_t)(V0 + t) * C;
        double max = -1000000000.0;
        for (int v = 0; v < V0; v++) {
            const double* x = w + (int64_t)v * C;
            double s = 0.0;
            for (int c = 0; c < C; c++) s += x[c] * y[c];
            expdot[(int64_t)t * V0 + v] = s;
            if (s > max) max = s;
        }
        for (int v = 0; v < V0; v++) {
            const double e = exp(expdot[(int64_t)t * V0 + v] - max);
            expdot[(int64_t)t * V0 + v] = e;
            sums[t] += e;
        }
    }
}
