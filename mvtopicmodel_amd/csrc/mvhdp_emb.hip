// mvhdp_emb.hip — word and topic embeddings (TopicWordEmbeddings / WordEmbeddings, TWE / TWER; PTM:337-367,517-524,1186-1206):
//   emb_init_kernel        weights = (u - 0.5) / C, negative weights 0 (TWE:143-148)
//   emb_count_kernel       the view-0 word counts of countWords (TWE:360-369)
//   emb_table_kernel       samplingTable (TWE:393-399): one lower_bound per index
//   emb_check_kernel       every view-0 token in [0, V_0), every z in [0, K) (before a train touches the weights)
//   emb_train_kernel       TWER:155-293 with gradientLearn TWER:82-152: one wave per entity, columns across lanes
//   emb_dot_kernel, emb_exp_kernel    CalcSoftmaxTopicWordProbabilities PTM:337-367
//   emb_cos_kernel         the cosines of findClosest TWE:485-540
// Stream contract: Philox4x32-10, counter (c0, 0x500 + purpose, global entity id, epoch), key (seed_lo ^ round,
// seed_hi); two 64-bit draws per call (words 0,1 then 2,3; draw n is call n >> 1).  Purposes: 0 subsampling (a uniform per original
// position), 1 window (nextInt(window) per kept position), 2 negatives (draw call * num_samples + s, skipped draws included),
// 3 initial weights (counter (col >> 1, 0x503, row, 0), key (seed_lo, seed_hi)).  No draw depends on the weights.
#include "mvhdp_ctx.h"
#include "mvhdp_wave.h"

namespace {

constexpr int EMB_MAXC = 256;                     // columns: at most 4 per lane
constexpr int EMB_NB = 6;                         // negatives whose dot products are reduced together with the positive one
constexpr int EMB_CAP = 512;                      // kept tokens per wave in LDS; a longer document spills to global scratch
constexpr int EMB_WPB = 4;                        // waves per block of the Hogwild trainer
constexpr int EMB_MAX_SAMPLES = 32;
constexpr uint32_t EMB_SUBSAMPLE = 0x500u, EMB_WINDOW = 0x501u, EMB_NEGATIVE = 0x502u, EMB_INIT = 0x503u;
enum { EC_WORDS = 0, EC_SAMPLED, EC_CONSIDERED, EC_SKIPPED, EC_CALLS, EC_NEGSKIP, EC_N };

__device__ __forceinline__ unsigned long long emb_draw64(uint32_t n, uint32_t purpose, uint32_t ent, uint32_t epoch, uint32_t k0, uint32_t k1)
{
    uint32_t x[4];
    philox4x32_10(n >> 1, purpose, ent, epoch, k0, k1, x);
    return (n & 1u) ? (((unsigned long long)x[2] << 32) | x[3]) : (((unsigned long long)x[0] << 32) | x[1]);
}
__device__ __forceinline__ double emb_unit(unsigned long long x) { return (double)(x >> 11) * 0x1.0p-53; }

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emb_init_kernel(double* __restrict__ w, double* __restrict__ neg, int64_t R, int C, uint32_t k0, uint32_t k1)
{
    const int64_t n = R * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        const double u = emb_unit(emb_draw64((uint32_t)c, EMB_INIT, (uint32_t)r, 0u, k0, k1));
        w[i] = (u - 0.5) / (double)C;                                                     // TWE:145
        neg[i] = 0.0;                                                                     // TWE:146
    }
}

__global__ __launch_bounds__(256) void emb_count_kernel(const int32_t* __restrict__ tok, int64_t N, int V, unsigned long long* __restrict__ cnt, int32_t* __restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = tok[i];
        if (t < 0 || t >= V) { atomicOr(err, 1); continue; }
        atomicAdd(&cnt[t], 1ull);                                                         // TWE:362
    }
}

// table[0] = sorted[0]; table[i] = sorted[first o with dist[o] >= S (i - 1) / size] (TWE:393-399: the while loop of index i - 1
// leaves `order` there), the product and the division in fp64 as written
__global__ __launch_bounds__(256) void emb_table_kernel(const double* __restrict__ dist, const int32_t* __restrict__ sorted, int V, double S,
                                                        int64_t size, int32_t* __restrict__ table)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += (int64_t)gridDim.x * blockDim.x) {
        int o = 0;
        if (i > 0) {
            const double x = S * (double)(i - 1) / (double)size;
            int lo = 0, hi = V - 1;                                                       // (dist[V - 1] = S >= x always)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (dist[mid] >= x) hi = mid; else lo = mid + 1; }
            o = lo;
        }
        table[i] = sorted[o];
    }
}

__global__ __launch_bounds__(256) void emb_check_kernel(const int32_t* __restrict__ tok, const int32_t* __restrict__ z, int64_t N, int V, int K, int32_t* __restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = tok[i];
        if (t < 0 || t >= V) atomicOr(err, 1);
        if (z) { const int k = z[i]; if (k < 0 || k >= K) atomicOr(err, 2); }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The trainer.  Lane l holds columns l, l + 64, l + 128, l + 192 of every row it touches.  A dot product is each lane's sum over its
// four columns in that order (from 0.0, a column outside the call's range adding 0.0 * 0.0), then the butterfly over lanes 32, 16, .., 1:
// every lane ends with the same bits, and tests/native/emb_ref.c restates exactly this order.
struct EmbArgs {
    const int64_t* doc_off; const int32_t* tok; const int32_t* z;     // view 0; z null without topics
    int64_t D, N0, total_words, ent_base;
    int V0, C, Cc, window, ns, min_len, epoch, epochs;
    int64_t table_size; const int32_t* table;
    const double* retention; const double* cache; int cache_size;
    double min_exp, max_exp, cache_scale;
    double* w; double* neg;
    int32_t* spill;                   // kept (token, topic) pairs beyond the first EMB_CAP of an entity, at 2 (spill_off[d] + i - EMB_CAP)
    const int64_t* spill_off;         // [D] prefix sums of max(0, length - EMB_CAP) (null: no entity that long)
    unsigned long long* queue;        // work-queue head (entities in id order)
    unsigned long long* ctr;          // [EC_N]
    double* res_part;                 // [waves] residual sum of each wave
    uint32_t k0, k1;
};

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

template <bool HOG>
__device__ __forceinline__ void emb_add(double* p, double v)
{
#ifndef MVHDP_EMB_PLAIN
    if (HOG) unsafeAtomicAdd(p, v);                           // memory-side fp64 add: no update lost between waves
    else
#endif
    *p += v;                                                  // (-DMVHDP_EMB_PLAIN: the measurement build of DESIGN.md §7b, plain stores everywhere)
}

struct EmbWave {
    int lane;
    uint32_t ent, call;
    double lr, res;
    unsigned long long calls, negskip;
};

template <bool HOG>
__device__ __forceinline__ void gradient_learn(const EmbArgs& a, const double* __restrict__ cache, EmbWave& s, int in, int out, bool ctx)
{
    const int lo = ctx ? 0 : a.Cc, hi = ctx ? a.Cc : a.C, lane = s.lane, C = a.C, ns = a.ns;
    double* const nin = a.neg + (int64_t)in * C;
    double* const wout = a.w + (int64_t)out * C;
    bool act[4];
    double wo[4], ni[4], gr[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int col = lane + 64 * j;
        act[j] = col >= lo && col < hi;
        wo[j] = act[j] ? wout[col] : 0.0;
        ni[j] = act[j] ? nin[col] : 0.0;
    }
    // the negatives of this call: lane q < ns draws number call * ns + q (TWER:118)
    int t = -1;
    if (lane < ns) {
        const unsigned long long x = emb_draw64(s.call * (uint32_t)ns + (uint32_t)lane, EMB_NEGATIVE, s.ent, (uint32_t)a.epoch, a.k0, a.k1);
        t = a.table[__umul64hi(x, (unsigned long long)a.table_size)];
    }
    s.call++;
    // the dots are reduced together when no kept negative repeats an earlier one: each then reads a row nothing in this call has written
    bool dup = false;
    for (int q = 0; q < ns; q++) { const int tq = __shfl(t, q, WAVE); if (q < lane && tq == t) dup = true; }
    const bool batch = ns <= EMB_NB && !__builtin_amdgcn_ballot_w64(lane < ns && t != in && dup);
    const double inv = 1.0 / ns;                                                          // oneOverNumSamples TWER:91
    auto resid = [&](double dot, bool positive) -> double {
        if (dot < a.min_exp) return positive ? s.lr : 0.0;                               // TWER:102-108, 130-136
        if (dot > a.max_exp) return positive ? 0.0 : -s.lr;
        const int ix = min(max((int)floor((dot - a.min_exp) * a.cache_scale), 0), a.cache_size);
        const double c = cache[ix];
        return positive ? s.lr * (1.0 - c) : s.lr * -c;
    };
    if (batch) {
        int tq[EMB_NB];
        double nt[EMB_NB][4], p[EMB_NB + 1];
        p[0] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) p[0] += ni[j] * wo[j];
#pragma unroll
        for (int q = 0; q < EMB_NB; q++) {
            tq[q] = __shfl(t, q < ns ? q : 0, WAVE);
            p[q + 1] = 0.0;
            const bool live = q < ns && tq[q] != in;
            const double* r = a.neg + (int64_t)(live ? tq[q] : 0) * C;
#pragma unroll
            for (int j = 0; j < 4; j++) { nt[q][j] = (live && act[j]) ? r[lane + 64 * j] : 0.0; p[q + 1] += nt[q][j] * wo[j]; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
            for (int q = 0; q <= EMB_NB; q++) p[q] += __shfl_xor(p[q], o, WAVE);
        double g = resid(p[0], true);
#pragma unroll
        for (int j = 0; j < 4; j++) { gr[j] = g * ni[j]; if (act[j]) emb_add<HOG>(&nin[lane + 64 * j], g * wo[j]); }   // TWER:110-113
        s.res += g;
#pragma unroll
        for (int q = 0; q < EMB_NB; q++) {
            if (q >= ns) break;
            if (tq[q] == in) { s.negskip++; continue; }                                   // TWER:119-121
            g = resid(p[q + 1], false);
            double* r = a.neg + (int64_t)tq[q] * C;
#pragma unroll
            for (int j = 0; j < 4; j++) { gr[j] += g * nt[q][j]; if (act[j]) emb_add<HOG>(&r[lane + 64 * j], g * wo[j]); }   // TWER:138-141
            s.res -= g * inv;
        }
    } else {
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) p += ni[j] * wo[j];
        p = wave_sum_d(p);
        double g = resid(p, true);
#pragma unroll
        for (int j = 0; j < 4; j++) { gr[j] = g * ni[j]; if (act[j]) emb_add<HOG>(&nin[lane + 64 * j], g * wo[j]); }
        s.res += g;
        for (int q = 0; q < ns; q++) {
            const int tt = __shfl(t, q, WAVE);
            if (tt == in) { s.negskip++; continue; }
            double* r = a.neg + (int64_t)tt * C;
            double nt[4];
            p = 0.0;
#pragma unroll
            for (int j = 0; j < 4; j++) { nt[j] = act[j] ? r[lane + 64 * j] : 0.0; p += nt[j] * wo[j]; }
            p = wave_sum_d(p);
            g = resid(p, false);
#pragma unroll
            for (int j = 0; j < 4; j++) { gr[j] += g * nt[j]; if (act[j]) emb_add<HOG>(&r[lane + 64 * j], g * wo[j]); }
            s.res -= g * inv;
        }
    }
    s.calls++;
#pragma unroll
    for (int j = 0; j < 4; j++) if (act[j]) emb_add<HOG>(&wout[lane + 64 * j], gr[j]);  // TWER:148-150
}

template <bool HOG>
__global__ __launch_bounds__(256) void emb_train_kernel(EmbArgs a)
{
    extern __shared__ unsigned char emb_lds[];
    double* cache = (double*)emb_lds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cache_n = a.cache_size + 1;
    int32_t* buf = (int32_t*)(emb_lds + (size_t)cache_n * 8) + (size_t)wave * 2 * EMB_CAP;   // [EMB_CAP] tokens, then [EMB_CAP] topics
    for (int i = threadIdx.x; i < cache_n; i += blockDim.x) cache[i] = a.cache[i];
    __syncthreads();
    const bool topics = a.z != nullptr;
    EmbWave s;
    s.lane = lane; s.res = 0.0; s.calls = 0; s.negskip = 0; s.ent = 0; s.call = 0; s.lr = 0.0;
    unsigned long long words = 0, sampled = 0, considered = 0, skipped = 0;
    const double lr_min = 0.025 * 0.0001;                                                 // TWER:221
    const double denom = (double)((int64_t)a.epochs * a.total_words);
    for (;;) {
        unsigned long long dd = 0;
        if (lane == 0) dd = atomicAdd(a.queue, 1ull);
        const int64_t d = (int64_t)__shfl(dd, 0, WAVE);
        if (d >= a.D) break;
        const int64_t b = a.doc_off[d];
        const int L = (int)(a.doc_off[d + 1] - b);
        s.ent = (uint32_t)(a.ent_base + d);
        s.call = 0;
        s.lr = fmax(lr_min, 0.025 * (1.0 - (double)((int64_t)a.epoch * a.N0 + b) / denom));   // constant per document
        int32_t* sp = a.spill_off ? a.spill + 2 * (a.spill_off[d] - EMB_CAP) : nullptr;   // (indexed from EMB_CAP on)
        // subsampling, 64 positions at a time: one uniform per original position (TWER:240-253), ballot compaction
        int len = 0;
        for (int base = 0; base < L; base += WAVE) {
            const int pos = base + lane;
            bool keep = false;
            int ty = 0, tk = 0;
            if (pos < L) {
                ty = a.tok[b + pos];
                tk = topics ? a.z[b + pos] : 0;
                keep = emb_unit(emb_draw64((uint32_t)pos, EMB_SUBSAMPLE, s.ent, (uint32_t)a.epoch, a.k0, a.k1)) < a.retention[ty];
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
            const int at = len + __popcll(m & ((1ull << lane) - 1ull));
            if (keep) {
                if (at < EMB_CAP) { buf[at] = ty; buf[EMB_CAP + at] = tk; }
                else { sp[2 * at] = ty; sp[2 * at + 1] = tk; }
            }
            len += __popcll(m);
        }
        words += L; sampled += len;
        if (len < a.min_len) { skipped++; continue; }                                    // TWER:256-259
        considered += len;
        if (len > EMB_CAP) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the spilled part, written by other lanes
        LDS_FENCE();
        auto tok_at = [&](int i) -> int { return i < EMB_CAP ? buf[i] : sp[2 * i]; };
        auto top_at = [&](int i) -> int { return i < EMB_CAP ? buf[EMB_CAP + i] : sp[2 * i + 1]; };
        for (int p = 0; p < len; p++) {
            const int in = tok_at(p);
            const int ta = a.V0 + top_at(p);
            if (topics) {
                gradient_learn<HOG>(a, cache, s, in, ta, true);                           // TWER:268
                gradient_learn<HOG>(a, cache, s, in, ta, false);                          // TWER:269
                gradient_learn<HOG>(a, cache, s, ta, in, false);                          // TWER:271
            }
            const int sw = (int)__umul64hi(emb_draw64((uint32_t)p, EMB_WINDOW, s.ent, (uint32_t)a.epoch, a.k0, a.k1), (unsigned long long)a.window) + 1;
            const int q0 = max(0, p - sw), q1 = min(len - 1, p + sw);                    // TWER:274-276
            for (int q = q0; q <= q1; q++) {
                if (q == p) continue;
                gradient_learn<HOG>(a, cache, s, in, tok_at(q), false);                   // TWER:284
                if (topics) gradient_learn<HOG>(a, cache, s, ta, a.V0 + top_at(q), true); // TWER:287
            }
        }
        LDS_FENCE();
    }
    if (lane == 0) {
        atomicAdd(&a.ctr[EC_WORDS], words); atomicAdd(&a.ctr[EC_SAMPLED], sampled); atomicAdd(&a.ctr[EC_CONSIDERED], considered);
        atomicAdd(&a.ctr[EC_SKIPPED], skipped); atomicAdd(&a.ctr[EC_CALLS], s.calls); atomicAdd(&a.ctr[EC_NEGSKIP], s.negskip);
        a.res_part[(int64_t)blockIdx.x * (blockDim.x >> 6) + wave] = s.res;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// softmax (PTM:337-367): dot[w][k] over the C columns in order (one thread per pair), then per topic the max, exp and the sum
__global__ __launch_bounds__(256) void emb_dot_kernel(const double* __restrict__ w, int V0, int K, int C, double* __restrict__ e)
{
    const int64_t n = (int64_t)V0 * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t wd = i / K;
        const int k = (int)(i - wd * K);
        const double* x = w + wd * C;
        const double* y = w + ((int64_t)V0 + k) * C;
        double s = 0.0;
        for (int c = 0; c < C; c++) s += x[c] * y[c];                                    // dotProduct(typeVectors[w], topicVectors[t])
        e[i] = s;
    }
}

// one block per topic: the max over the words (PTM:342-352, from -1e9), exp in place (PTM:358-359), the sum in a fixed order
__global__ __launch_bounds__(256) void emb_exp_kernel(double* __restrict__ e, int V0, int K, double* __restrict__ sums)
{
    __shared__ double red[256];
    const int k = blockIdx.x;
    double mx = -1000000000.0;
    for (int wd = threadIdx.x; wd < V0; wd += blockDim.x) { const double v = e[(int64_t)wd * K + k]; if (v > mx) mx = v; }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s]; __syncthreads(); }
    mx = red[0];
    __syncthreads();
    double sum = 0.0;
    for (int wd = threadIdx.x; wd < V0; wd += blockDim.x) {
        const int64_t i = (int64_t)wd * K + k;
        const double x = exp(e[i] - mx);
        e[i] = x;
        sum += x;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) sums[k] = red[0];
}

// [V0][K] -> [K][V0] (the copy a caller asks for)
__global__ __launch_bounds__(256) void emb_transpose_kernel(const double* __restrict__ e, int V0, int K, double* __restrict__ out)
{
    __shared__ double tile[32][33];
    const int w0 = blockIdx.x * 32, k0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) { const int wd = w0 + r, k = k0 + tx; tile[r][tx] = (wd < V0 && k < K) ? e[(int64_t)wd * K + k] : 0.0; }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) { const int k = k0 + r, wd = w0 + tx; if (k < K && wd < V0) out[(int64_t)k * V0 + wd] = tile[tx][r]; }
}

// findClosest TWE:487-541: innerProduct * (targetNormalizer * wordNormalizer), every sum over the C columns in order
__global__ __launch_bounds__(256) void emb_cos_kernel(const double* __restrict__ w, int64_t R, int C, const double* __restrict__ q, double* __restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const double* x = w + r * C;
        double tq = 0.0, sq = 0.0, ip = 0.0;
        for (int c = 0; c < C; c++) tq += q[c] * q[c];
        for (int c = 0; c < C; c++) sq += x[c] * x[c];
        for (int c = 0; c < C; c++) ip += q[c] * x[c];
        const double tn = 1.0 / sqrt(tq), wn = 1.0 / sqrt(sq);
        ip *= tn * wn;
        out[r] = ip;
    }
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// the state on the handle (mvhdp_ctx::emb)
// ---------------------------------------------------------------------------------------------------------------
struct EmbState {
    mvhdp_emb_config cfg{};
    int64_t R = 0;
    int V0 = 0, K = 0, Cc = 0;
    double* w = nullptr;                  // [R][C] weights
    double* neg = nullptr;                // [R][C] negativeWeights
    double* cache = nullptr;              // [cache_size + 1] sigmoidCache
    std::vector<int64_t> counts;          // cumulative wordCounts (TWE:362)
    int64_t total_words = 0;              // cumulative totalWords (TWE:369)
    std::vector<double> retention;
    double* d_retention = nullptr;
    int32_t* table = nullptr;             // [sampling_table_size]
    bool have_table = false;
    int32_t* spill = nullptr;             // [2 x the tokens beyond EMB_CAP of the long entities] when an entity is longer than EMB_CAP
    int64_t spill_n = 0;
    int64_t* spill_off = nullptr;         // [D]
    int64_t spill_off_n = 0;
    double* expdot = nullptr;             // [V0][K] exp(dot - max): p_emb(w|t) = expdot / sum_exp, gathered beside n_wk by the λ mix
    std::vector<double> sum_exp;          // [K] accumulated over softmax calls (PTM:360)
    unsigned long long* ctl = nullptr;    // [1 + EC_N] queue head, counters
    double* res_part = nullptr;
    int res_n = 0;
};

void mvhdp_emb_free(mvhdp_ctx* h)
{
    EmbState* e = h->emb;
    if (!e) return;
    auto fr = [](auto*& p) { if (p) { hipFree((void*)p); p = nullptr; } };
    fr(e->w); fr(e->neg); fr(e->cache); fr(e->d_retention); fr(e->table); fr(e->spill); fr(e->spill_off); fr(e->expdot); fr(e->ctl); fr(e->res_part);
    delete e;
    h->emb = nullptr;
}

bool mvhdp_emb_has_topic_rows(const mvhdp_ctx* h) { return h->emb && h->emb->K > 0; }

static int emb_ready(mvhdp_ctx* h)
{
    if (!h->emb) FAIL(h, MVHDP_ERR_STATE, "embeddings: mvhdp_emb_init has not been called");
    return MVHDP_OK;
}

static int emb_init_state(mvhdp_ctx* h, const mvhdp_emb_config& c, const double* weights, uint64_t seed)
{
    EmbState* e = h->emb;
    e->cfg = c;
    e->V0 = h->mm.V[0];
    e->K = c.with_topics ? h->mm.K : 0;
    e->Cc = c.with_topics ? c.num_context_columns : 0;                                   // TWE:136
    e->R = (int64_t)e->V0 + e->K;
    const int C = c.num_columns;
    const size_t nb = (size_t)e->R * C * sizeof(double);
    HIPC(h, hipMalloc(&e->w, nb));
    HIPC(h, hipMalloc(&e->neg, nb));
    // sigmoidCache TWE:157-162 on the host with the reference's expression; cache[size] is never set (0.0)
    const int S = c.sigmoid_cache_size;
    std::vector<double> cache((size_t)S + 1, 0.0);
    for (int i = 0; i < S; i++) {
        const double value = ((double)i / S) * (c.max_exp - c.min_exp) + c.min_exp;
        cache[i] = 1.0 / (1.0 + std::exp(-value));
    }
    HIPC(h, hipMalloc(&e->cache, cache.size() * sizeof(double)));
    HIPC(h, hipMemcpy(e->cache, cache.data(), cache.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMalloc(&e->ctl, (1 + EC_N) * sizeof(unsigned long long)));
    e->counts.assign((size_t)e->V0, 0);
    if (weights) {
        HIPC(h, hipMemcpy(e->w, weights, nb, hipMemcpyHostToDevice));
        HIPC(h, hipMemset(e->neg, 0, nb));
    } else {
        LAUNCH(h, emb_init_kernel, dim3(grid_for(e->R * C)), dim3(256), 0, h->stream, e->w, e->neg, e->R, C, (uint32_t)seed, (uint32_t)(seed >> 32));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_init(mvhdp_handle h, const mvhdp_emb_config* cfg, const double* weights, uint64_t seed)
{
    CHECK_H(h);
    if (!cfg) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: null config");
    const mvhdp_emb_config& c = *cfg;
    if (c.num_columns < 1 || c.num_columns > EMB_MAXC) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: num_columns must be 1..256");
    if (c.num_context_columns < 0 || c.num_context_columns >= c.num_columns) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: 0 <= num_context_columns < num_columns");
    if (c.window < 1 || c.num_samples < 0 || c.num_samples > EMB_MAX_SAMPLES || c.min_doc_length < 1)
        FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: window >= 1, num_samples 0..32, min_doc_length >= 1");
    if (c.sampling_table_size < 1 || c.sampling_table_size > INT32_MAX) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: sampling_table_size must be 1..2^31-1");
    if (!(c.sampling_factor > 0.0) || !(c.max_exp > c.min_exp) || c.sigmoid_cache_size < 1 || c.sigmoid_cache_size > 4096)
        FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_init: sampling_factor > 0, min_exp < max_exp, sigmoid_cache_size 1..4096");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    mvhdp_emb_free(h);
    h->emb = new EmbState();
    const int rc = emb_init_state(h, c, weights, seed);
    if (rc) mvhdp_emb_free(h);
    return rc;
}

extern "C" int mvhdp_emb_count_words(mvhdp_handle h)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    if (!h->have_corpus[0]) FAIL(h, MVHDP_ERR_STATE, "emb_count_words: no view-0 corpus (set_corpus)");
    EmbState* e = h->emb;
    const int V0 = e->V0;
    const int64_t N0 = h->N[0];
    if (N0 <= 0) FAIL(h, MVHDP_ERR_STATE, "emb_count_words: no view-0 tokens");
    HIPC(h, hipSetDevice(h->device));
    std::vector<unsigned long long> cnt((size_t)V0, 0);
    int32_t err = 0;
    {
        DevArray<unsigned long long> d_cnt;
        DevArray<int32_t> d_err;
        HIPC(h, d_cnt.alloc((size_t)V0)); HIPC(h, d_err.alloc(1));
        HIPC(h, d_cnt.fill(0, h->stream));
        HIPC(h, d_err.fill(0, h->stream));
        LAUNCH(h, emb_count_kernel, dim3(grid_for(N0)), dim3(256), 0, h->stream, h->mm.tok[0], N0, V0, d_cnt, d_err);
        HIPC(h, d_cnt.download(cnt.data(), (size_t)V0, h->stream));
        HIPC(h, d_err.download(&err, 1, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    if (err) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_count_words: a view-0 token is outside [0, V_0)");
    // TWE:362,369: cumulative over calls (kept quirk); committed to the handle only once the table below is built, so a failed call
    // leaves the counts as they were and a retry does not count the corpus twice
    std::vector<int64_t> counts(e->counts);
    for (int w = 0; w < V0; w++) counts[w] += (int64_t)cnt[w];
    const int64_t total_words = e->total_words + N0;
    const double f = e->cfg.sampling_factor;
    std::vector<double> retention((size_t)V0, 0.0);
    for (int w = 0; w < V0; w++) {                                                       // TWE:373-377
        const double s = (double)counts[w] / (f * (double)total_words);
        const double r = (std::sqrt(s) + 1) / s;
        retention[w] = r < 1.0 ? r : 1.0;
    }
    std::vector<int32_t> sorted((size_t)V0);                                             // TWE:379-385: IDSorter order
    for (int w = 0; w < V0; w++) sorted[w] = w;
    std::sort(sorted.begin(), sorted.end(), [&](int32_t x, int32_t y) { return counts[x] != counts[y] ? counts[x] > counts[y] : x > y; });
    std::vector<double> dist((size_t)V0);
    dist[0] = std::pow((double)counts[sorted[0]], 0.75);                                 // TWE:387-391
    for (int w = 1; w < V0; w++) dist[w] = dist[w - 1] + std::pow((double)counts[sorted[w]], 0.75);
    const int64_t size = e->cfg.sampling_table_size;
    if (!e->d_retention) HIPC(h, hipMalloc(&e->d_retention, (size_t)V0 * sizeof(double)));
    if (!e->table) HIPC(h, hipMalloc(&e->table, (size_t)size * sizeof(int32_t)));
    e->have_table = false;                                                               // (the table and retention are rewritten below)
    HIPC(h, hipMemcpyAsync(e->d_retention, retention.data(), (size_t)V0 * 8, hipMemcpyHostToDevice, h->stream));
    {
        DevArray<double> d_dist;
        DevArray<int32_t> d_sorted;
        HIPC(h, d_dist.alloc((size_t)V0)); HIPC(h, d_sorted.alloc((size_t)V0));
        HIPC(h, d_dist.upload(dist.data(), (size_t)V0, h->stream));
        HIPC(h, d_sorted.upload(sorted.data(), (size_t)V0, h->stream));
        LAUNCH(h, emb_table_kernel, dim3(grid_for(size)), dim3(256), 0, h->stream, d_dist, d_sorted, V0, dist[V0 - 1], size, e->table);
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    e->counts.swap(counts);
    e->total_words = total_words;
    e->retention.swap(retention);
    e->have_table = true;
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_train(mvhdp_handle h, int32_t epochs, uint64_t seed, uint32_t round, uint32_t flags, mvhdp_emb_stats* stats)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    if (epochs < 1) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_train: epochs must be >= 1");
    if (flags & ~MVHDP_EMB_SERIAL) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_train: unknown flags");
    if (!h->have_corpus[0]) FAIL(h, MVHDP_ERR_STATE, "emb_train: no view-0 corpus (set_corpus)");
    if (!e->have_table) FAIL(h, MVHDP_ERR_STATE, "emb_train: mvhdp_emb_count_words has not been called");
    MvModel& mm = h->mm;
    const int64_t N0 = h->N[0], D = mm.D;
    const bool topics = e->K > 0;
    HIPC(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    {   // every token and topic in range first: a refused call leaves the vectors as they were
        DevArray<int32_t> d_err;
        int32_t err = 0;
        HIPC(h, d_err.alloc(1));
        HIPC(h, d_err.fill(0, st));
        if (N0 > 0)
            LAUNCH(h, emb_check_kernel, dim3(grid_for(N0)), dim3(256), 0, st, mm.tok[0], topics ? (const int32_t*)mm.z[0] : nullptr, N0, e->V0, mm.K, d_err);
        HIPC(h, d_err.download(&err, 1, st));
        HIPC(h, hipStreamSynchronize(st));
        if (err & 1) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_train: a view-0 token is outside [0, V_0)");
        if (err & 2) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_train: a view-0 topic is unassigned or outside [0, K)");
    }
    // the tokens an entity keeps beyond the LDS buffer go to global scratch: the tails of the long entities, packed
    const std::vector<int64_t>& off = h->h_doc_off[0];
    std::vector<int64_t> tail((size_t)std::max<int64_t>(D, 1), 0);
    int64_t tails = 0;
    for (int64_t d = 0; d < D; d++) { tail[d] = tails; tails += std::max<int64_t>(0, off[d + 1] - off[d] - EMB_CAP); }
    if (tails > 0) {
        if (e->spill_n < tails) {
            if (e->spill) { hipFree(e->spill); e->spill = nullptr; e->spill_n = 0; }
            HIPC(h, hipMalloc(&e->spill, (size_t)tails * 2 * sizeof(int32_t)));
            e->spill_n = tails;
        }
        if (e->spill_off_n < D) {
            if (e->spill_off) { hipFree(e->spill_off); e->spill_off = nullptr; e->spill_off_n = 0; }
            HIPC(h, hipMalloc(&e->spill_off, (size_t)D * sizeof(int64_t)));
            e->spill_off_n = D;
        }
        HIPC(h, hipMemcpyAsync(e->spill_off, tail.data(), (size_t)D * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    const bool serial = (flags & MVHDP_EMB_SERIAL) != 0;
    const size_t lds = (size_t)(e->cfg.sigmoid_cache_size + 1) * 8 + (size_t)EMB_WPB * 2 * EMB_CAP * 4;
    int grid = 1, block = 64;
    if (!serial) {
        block = 64 * EMB_WPB;
        grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->num_cus * 8, (D + EMB_WPB - 1) / EMB_WPB));
    }
    const int waves = grid * (block / 64);
    if (e->res_n < waves) {
        if (e->res_part) { hipFree(e->res_part); e->res_part = nullptr; e->res_n = 0; }
        HIPC(h, hipMalloc(&e->res_part, (size_t)waves * sizeof(double)));
        e->res_n = waves;
    }
    EmbArgs a{};
    a.doc_off = mm.doc_off[0]; a.tok = mm.tok[0]; a.z = topics ? mm.z[0] : nullptr;
    a.D = D; a.N0 = N0; a.total_words = e->total_words; a.ent_base = mm.doc_id_base;
    a.V0 = e->V0; a.C = e->cfg.num_columns; a.Cc = e->Cc; a.window = e->cfg.window; a.ns = e->cfg.num_samples; a.min_len = e->cfg.min_doc_length;
    a.epochs = epochs;
    a.table_size = e->cfg.sampling_table_size; a.table = e->table;
    a.retention = e->d_retention; a.cache = e->cache; a.cache_size = e->cfg.sigmoid_cache_size;
    a.min_exp = e->cfg.min_exp; a.max_exp = e->cfg.max_exp;
    a.cache_scale = (double)e->cfg.sigmoid_cache_size / (e->cfg.max_exp - e->cfg.min_exp);   // TWER:92
    a.w = e->w; a.neg = e->neg; a.spill = tails > 0 ? e->spill : nullptr; a.spill_off = tails > 0 ? e->spill_off : nullptr;
    a.queue = e->ctl; a.ctr = e->ctl + 1; a.res_part = e->res_part;
    a.k0 = (uint32_t)seed ^ round; a.k1 = (uint32_t)(seed >> 32);
    const void* fn = serial ? (const void*)emb_train_kernel<false> : (const void*)emb_train_kernel<true>;
    HIPC(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPC(h, hipMemsetAsync(e->ctl + 1, 0, EC_N * sizeof(unsigned long long), st));
    double residual = 0.0, last = 0.0, kernel_ms = 0.0;
    unsigned long long ctr[EC_N] = {}, prev_calls = 0, last_calls = 0;
    std::vector<double> part((size_t)waves);
    for (int ep = 0; ep < epochs; ep++) {                                                // epochs in order, one launch each
        a.epoch = ep;
        HIPC(h, hipMemsetAsync(e->ctl, 0, sizeof(unsigned long long), st));
        HIPC(h, hipEventRecord(h->ev[0], st));
        if (serial) LAUNCH(h, emb_train_kernel<false>, dim3(grid), dim3(block), lds, st, a);
        else LAUNCH(h, emb_train_kernel<true>, dim3(grid), dim3(block), lds, st, a);
        HIPC(h, hipEventRecord(h->ev[1], st));
        HIPC(h, hipMemcpyAsync(part.data(), e->res_part, (size_t)waves * 8, hipMemcpyDeviceToHost, st));
        HIPC(h, hipMemcpyAsync(ctr, e->ctl + 1, sizeof(ctr), hipMemcpyDeviceToHost, st));
        HIPC(h, hipStreamSynchronize(st));
        float ms = 0.f;
        HIPC(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        kernel_ms += ms;                                                                 // the training launches alone
        double r = 0.0;
        for (int i = 0; i < waves; i++) r += part[i];                                   // wave order
        residual += r;
        last = r;
        last_calls = ctr[EC_CALLS] - prev_calls;
        prev_calls = ctr[EC_CALLS];
    }
    if (stats) {
        stats->words_so_far = (int64_t)ctr[EC_WORDS]; stats->words_sampled = (int64_t)ctr[EC_SAMPLED];
        stats->words_considered = (int64_t)ctr[EC_CONSIDERED]; stats->docs_skipped = (int64_t)ctr[EC_SKIPPED];
        stats->calls = (int64_t)ctr[EC_CALLS]; stats->negatives_skipped = (int64_t)ctr[EC_NEGSKIP];
        stats->residual = residual; stats->last_epoch_residual = last; stats->last_epoch_calls = (int64_t)last_calls;
        stats->kernel_ms = kernel_ms;
    }
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_get_vectors(mvhdp_handle h, double* weights, double* negative_weights)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    const size_t nb = (size_t)e->R * e->cfg.num_columns * sizeof(double);
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (weights) HIPC(h, hipMemcpy(weights, e->w, nb, hipMemcpyDeviceToHost));
    if (negative_weights) HIPC(h, hipMemcpy(negative_weights, e->neg, nb, hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_set_vectors(mvhdp_handle h, const double* weights, const double* negative_weights)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    const size_t nb = (size_t)e->R * e->cfg.num_columns * sizeof(double);
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (weights) HIPC(h, hipMemcpy(e->w, weights, nb, hipMemcpyHostToDevice));
    if (negative_weights) HIPC(h, hipMemcpy(e->neg, negative_weights, nb, hipMemcpyHostToDevice));
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_word_stats(mvhdp_handle h, int64_t* counts, double* retention, int64_t* total_words)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    if (!e->have_table) FAIL(h, MVHDP_ERR_STATE, "emb_word_stats: mvhdp_emb_count_words has not been called");
    if (counts) std::copy(e->counts.begin(), e->counts.end(), counts);
    if (retention) std::copy(e->retention.begin(), e->retention.end(), retention);
    if (total_words) *total_words = e->total_words;
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_sampling_table(mvhdp_handle h, int64_t first, int64_t n, int32_t* types)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    if (!e->have_table) FAIL(h, MVHDP_ERR_STATE, "emb_sampling_table: mvhdp_emb_count_words has not been called");
    if (!types || first < 0 || n < 0 || first + n > e->cfg.sampling_table_size) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_sampling_table: range outside the table");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (n > 0) HIPC(h, hipMemcpy(types, e->table + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_softmax(mvhdp_handle h, int32_t reset_sums, double* exp_dot, double* sum_exp)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    if (e->K == 0) FAIL(h, MVHDP_ERR_STATE, "emb_softmax: the embeddings have no topic rows (with_topics = 0)");
    const int V0 = e->V0, K = e->K, C = e->cfg.num_columns;
    HIPC(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    if (!e->expdot) HIPC(h, hipMalloc(&e->expdot, (size_t)V0 * K * sizeof(double)));
    std::vector<double> sums((size_t)K);
    {
        DevArray<double> d_sums, d_t;
        HIPC(h, d_sums.alloc((size_t)K));
        LAUNCH(h, emb_dot_kernel, dim3(grid_for((int64_t)V0 * K)), dim3(256), 0, st, e->w, V0, K, C, e->expdot);
        LAUNCH(h, emb_exp_kernel, dim3(K), dim3(256), 0, st, e->expdot, V0, K, d_sums);
        HIPC(h, d_sums.download(sums.data(), (size_t)K, st));
        if (exp_dot) {
            HIPC(h, d_t.alloc((size_t)V0 * K));
            LAUNCH(h, emb_transpose_kernel, dim3((V0 + 31) / 32, (K + 31) / 32), dim3(256), 0, st, e->expdot, V0, K, d_t);
            HIPC(h, d_t.download(exp_dot, (size_t)V0 * K, st));
        }
        HIPC(h, hipStreamSynchronize(st));
    }
    if (reset_sums || e->sum_exp.size() != (size_t)K) e->sum_exp.assign((size_t)K, 0.0);
    for (int k = 0; k < K; k++) e->sum_exp[k] += sums[k];                               // PTM:360, never reset by the reference
    if (sum_exp) std::copy(e->sum_exp.begin(), e->sum_exp.end(), sum_exp);
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_nearest(mvhdp_handle h, const double* query, int32_t n, int32_t* words, double* word_sims, int32_t* topics, double* topic_sims)
{
    CHECK_H(h);
    int rc = emb_ready(h); if (rc) return rc;
    EmbState* e = h->emb;
    if (!query || !words || !word_sims) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_nearest: null query or word output");
    if (n < 1 || n > 64) FAIL(h, MVHDP_ERR_INVALID_ARG, "emb_nearest: n must be 1..64");
    const int C = e->cfg.num_columns;
    HIPC(h, hipSetDevice(h->device));
    std::vector<double> sim((size_t)e->R);
    {
        DevArray<double> d_q, d_s;
        HIPC(h, d_q.alloc((size_t)C)); HIPC(h, d_s.alloc((size_t)e->R));
        HIPC(h, d_q.upload(query, (size_t)C, h->stream));
        LAUNCH(h, emb_cos_kernel, dim3(grid_for(e->R)), dim3(256), 0, h->stream, e->w, e->R, C, d_q, d_s);
        HIPC(h, d_s.download(sim.data(), (size_t)e->R, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    // IDSorter order (weight descending, equal weights by descending id), cut at n: a partial sort of V_0 + K values on the host
    auto top = [&](int64_t base, int cnt, int32_t* ids, double* sims) {
        std::vector<int32_t> idx((size_t)cnt);
        for (int i = 0; i < cnt; i++) idx[i] = i;
        const int m = std::min(n, cnt);
        std::partial_sort(idx.begin(), idx.begin() + m, idx.end(), [&](int32_t x, int32_t y) {
            const double p = sim[base + x], q = sim[base + y];
            return p != q ? p > q : x > y;
        });
        for (int i = 0; i < n; i++) { ids[i] = i < m ? idx[i] : -1; sims[i] = i < m ? sim[base + idx[i]] : std::numeric_limits<double>::quiet_NaN(); }
    };
    top(0, e->V0, words, word_sims);
    if (e->K > 0 && topics && topic_sims) top(e->V0, e->K, topics, topic_sims);
    return MVHDP_OK;
}

extern "C" int mvhdp_emb_release(mvhdp_handle h)
{
    CHECK_H(h);
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    mvhdp_emb_free(h);
    return MVHDP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The useVectorsLambda mix of the sweep (PTM:1199-1207 hands the tables to the workers; WRK:504-507, PTM:2673-2678, UPD:244-260 use them):
// the handle's own table mix[w][k] = lambda * (e[k][w] / S[k]) -- the first product of the reference's expression, its two operations in
// the reference's order, each correctly rounded -- in the layout of the view-0 rows of n_wk.  The samplers and the tree kernel add
// (1 - lambda) * the count ratio (MvModel::mix, MvModel::oml).
// ---------------------------------------------------------------------------------------------------------------
// e in the reference's layout [K][V0] (a host's tables)
__global__ __launch_bounds__(256) void mix_from_kv_kernel(const double* __restrict__ e, const double* __restrict__ S, double lambda, int V0, int K, double* __restrict__ mix, float* __restrict__ mix32, unsigned int* __restrict__ bad)
{
    const int64_t n = (int64_t)V0 * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t w = i / K;
        const int k = (int)(i - w * K);
        const double v = lambda * (e[(int64_t)k * V0 + w] / S[k]);
        mix[i] = v; mix32[i] = (float)v;
        if (!(v >= 0.0 && v <= 1.7e308 && (double)(float)v <= 3.4e38)) atomicOr(bad, 1u);   // (a finite e over a tiny S: the quotient is checked, not only its parts)
    }
}
// e as mvhdp_emb_softmax keeps it, [V0][K]
__global__ __launch_bounds__(256) void mix_from_vk_kernel(const double* __restrict__ e, const double* __restrict__ S, double lambda, int V0, int K, double* __restrict__ mix, float* __restrict__ mix32, unsigned int* __restrict__ bad)
{
    const int64_t n = (int64_t)V0 * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = lambda * (e[i] / S[i % K]);
        mix[i] = v; mix32[i] = (float)v;
        if (!(v >= 0.0 && v <= 1.7e308 && (double)(float)v <= 3.4e38)) atomicOr(bad, 1u);
    }
}

extern "C" int mvhdp_set_vectors_mix(mvhdp_handle h, double lambda, const double* exp_dot, const double* sum_exp)
{
    CHECK_H(h);
    if (!(lambda >= 0.0 && lambda <= 1.0)) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_vectors_mix: lambda outside [0, 1]");
    if ((exp_dot == nullptr) != (sum_exp == nullptr)) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_vectors_mix: exp_dot and sum_exp go together (both, or both NULL)");
    if (h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "set_vectors_mix: an mvhdp_apply_delta_begin bracket is open");
    const int V0 = h->mm.V[0], K = h->mm.K;
    const size_t n = (size_t)V0 * K;
    HIPC(h, hipSetDevice(h->device));
    if (lambda == 0.0) {                                        // off: the state after mvhdp_create
        HIPC(h, hipStreamSynchronize(h->stream));
        if (h->d_mix) { hipFree(h->d_mix); h->d_mix = nullptr; }
        if (h->d_mix32) { hipFree(h->d_mix32); h->d_mix32 = nullptr; }
        h->mm.mix = nullptr; h->mm.mix32 = nullptr; h->mm.oml = 1.0; h->mix_lambda = 0.0;
        h->st.trees_outdated();
        return MVHDP_OK;
    }
    const double* S_host = sum_exp;
    if (!exp_dot) {
        EmbState* e = h->emb;
        if (!e || !e->expdot || e->sum_exp.size() != (size_t)K || e->V0 != V0)
            FAIL(h, MVHDP_ERR_STATE, "set_vectors_mix: no softmax table on the handle (mvhdp_emb_softmax has not been called)");
        S_host = e->sum_exp.data();
    } else {
        for (size_t i = 0; i < n; i++) if (!(exp_dot[i] >= 0.0) || !std::isfinite(exp_dot[i])) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_vectors_mix: an exp_dot entry is negative or not finite");
    }
    for (int k = 0; k < K; k++) if (!(S_host[k] > 0.0) || !std::isfinite(S_host[k])) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_vectors_mix: a sum_exp entry is not a positive finite number");
    // everything checked: from here on the new table replaces the old one
    DevArray<double> d_S, d_e, d_new;
    DevArray<float> d_new32;
    DevArray<unsigned int> d_bad;
    unsigned int h_bad = 0;
    HIPC(h, d_S.alloc((size_t)K));
    if (exp_dot) HIPC(h, d_e.alloc(n));
    HIPC(h, d_new.alloc(n));
    HIPC(h, d_new32.alloc(n + 4));                             // 16 bytes of slack behind the fp32 table
    HIPC(h, d_bad.alloc(1));
    const hipStream_t st = h->stream;
    HIPC(h, d_bad.fill(0, st));
    HIPC(h, d_S.upload(S_host, (size_t)K, st));
    if (exp_dot) {
        HIPC(h, d_e.upload(exp_dot, n, st));
        LAUNCH(h, mix_from_kv_kernel, dim3(grid_for((int64_t)n)), dim3(256), 0, st, d_e, d_S, lambda, V0, K, d_new, d_new32, d_bad);
    } else
        LAUNCH(h, mix_from_vk_kernel, dim3(grid_for((int64_t)n)), dim3(256), 0, st, h->emb->expdot, d_S, lambda, V0, K, d_new, d_new32, d_bad);
    HIPC(h, d_bad.download(&h_bad, 1, st));
    HIPC(h, hipStreamSynchronize(st));
    // the mix in force stays as it is
    if (h_bad) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_vectors_mix: lambda * (exp_dot / sum_exp) is not finite (or beyond fp32's range) for some cell");
    if (h->d_mix) hipFree(h->d_mix);
    if (h->d_mix32) hipFree(h->d_mix32);
    h->d_mix = d_new.release(); h->d_mix32 = d_new32.release();
    h->mm.mix = h->d_mix; h->mm.mix32 = h->d_mix32; h->mm.oml = 1.0 - lambda; h->mix_lambda = lambda;
    h->st.trees_outdated();
    return MVHDP_OK;
}

extern "C" int mvhdp_get_vectors_mix(mvhdp_handle h, double* lambda, double* mix)
{
    CHECK_H(h);
    if (lambda) *lambda = h->mix_lambda;
    if (mix) {
        if (!h->d_mix) FAIL(h, MVHDP_ERR_STATE, "get_vectors_mix: no mix is set");
        HIPC(h, hipSetDevice(h->device));
        HIPC(h, hipStreamSynchronize(h->stream));
        HIPC(h, hipMemcpy(mix, h->d_mix, (size_t)h->mm.V[0] * h->mm.K * sizeof(double), hipMemcpyDeviceToHost));
    }
    return MVHDP_OK;
}
