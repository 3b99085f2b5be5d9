// mvhdp_diag.hip — the topic diagnostics that follow training (FastQMVWVTopicModelDiagnostics, DIAG; PTM:1792-1811, 2181-2270):
//   diag_transpose_kernel   n_wk of one view -> [K][V_m], so that every topic's column is contiguous
//   diag_rows_kernel        typeDiscrWeight of calcDiscrWeightAcrossTopicsPerModality (PTM:2193-2221): one wave per n_wk row
//   diag_topn_kernel        getSortedWords (PTM:1792-1811) cut at n: one block per topic, a sorted top-64 list per wave in registers
//   diag_doc_kernel         collectDocumentStatistics (DIAG:120-236) over view 0: one wave per entity
//   diag_sum_partials       the per-wave sums of c log c (DIAG:196), added in wave order
//   diag_columns_kernel     the K x V_0 column sums of uniform_dist, corpus_dist, eff_num_words and discrWeight (DIAG:262-404, PTM:2243-2262)
// Integer outputs are exact.  No floating-point atomics anywhere: every fp64 sum is a per-thread / per-wave sum over a static share
// of the work followed by a reduction in a fixed order, so the same model gives the same bits on every call.
#include "mvhdp_side.h"
#include "mvhdp_select.h"

namespace {

constexpr int DIAG_NPROP = MVHDP_DIAG_PROPORTIONS;
__constant__ double c_doc_proportions[DIAG_NPROP] = {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5};      // DIAG:27
constexpr int ROWS_BLOCKS = 512;                   // fixed: the summation order of skewSum is part of the result
constexpr int DOC_WAVES = 4096;                    // waves of the document pass (c log c partials: one [K] row each)
constexpr int NCOL = 7;                            // diag_columns_kernel outputs per topic

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diag_transpose_kernel(const int32_t* __restrict__ nwk, int V, int K, int32_t* __restrict__ nkw)
{
    __shared__ int32_t tile[64][65];
    const int w0 = blockIdx.x * 64, k0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int w = w0 + r, k = k0 + tx;
        tile[r][tx] = (w < V && k < K) ? nwk[(int64_t)w * K + k] : 0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, w = w0 + tx;
        if (k < K && w < V) nkw[(int64_t)k * V + w] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// PTM:2196-2220 for the rows [0, V) of one view: tw[w] = sum_k c^2 / (sum_k c)^2 (0 for an empty row), rowsum[w] = sum_k c.
// part[b] = (sum of the tw > 0 of block b's rows, their number); a wave's rows in ascending order, the four waves in order.
__global__ __launch_bounds__(256) void diag_rows_kernel(const int32_t* __restrict__ nwk, int V, int K, double* __restrict__ tw,
                                                        int64_t* __restrict__ rowsum, double* __restrict__ part_sum, long long* __restrict__ part_cnt)
{
    __shared__ double ss[4];
    __shared__ long long sc[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    long long n = 0;
    for (int w = blockIdx.x * 4 + wave; w < V; w += gridDim.x * 4) {
        const int32_t* row = nwk + (int64_t)w * K;
        long long sq = 0, tot = 0;
        for (int k = lane; k < K; k += WAVE) { const long long c = row[k]; sq += c * c; tot += c; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { sq += __shfl_xor(sq, o, WAVE); tot += __shfl_xor(tot, o, WAVE); }
        const double t = tot > 0 ? (double)sq / ((double)tot * (double)tot) : 0.0;        // PTM:2207,2214
        if (lane == 0) { tw[w] = t; rowsum[w] = tot; }
        if (t > 0) { s += t; n++; }                                                       // PTM:2216-2219
    }
    if (lane == 0) { ss[wave] = s; sc[wave] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
        part_cnt[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Top n of one topic's column (IDSorter order: count descending, equal counts by descending type id).  A key (count << 32 | type)
// orders exactly so; every lane of a wave holds one entry of the wave's sorted list (lane i: the i-th largest so far), a key enters
// only when it beats the n-th, by one ballot and one shuffle (topn_offer, mvhdp_select.h).  The four waves' lists are merged by wave 0.
__global__ __launch_bounds__(256) void diag_topn_kernel(const int32_t* __restrict__ nkw, int V, int n, int32_t* __restrict__ types,
                                                        int32_t* __restrict__ counts, int32_t* __restrict__ nonzero)
{
    __shared__ unsigned long long lists[4][64];
    __shared__ int nzs[4];
    const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* col = nkw + (int64_t)k * V;
    const int per = (V + 3) / 4, b = wave * per, e = min(V, b + per);
    unsigned long long list = 0, thr = 0;
    int nz = 0;
    for (int base = b; base < e; base += WAVE) {
        const int w = base + lane;
        unsigned long long key = 0;
        if (w < e) { const int c = col[w]; if (c > 0) { nz++; key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)w; } }
        if (__builtin_amdgcn_ballot_w64(key > thr)) topn_offer(list, thr, key, n, lane, KeyDescending());
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nz += __shfl_xor(nz, o, WAVE);
    lists[wave][lane] = list;
    if (lane == 0) nzs[wave] = nz;
    __syncthreads();
    if (wave != 0) return;
    for (int w2 = 1; w2 < 4; w2++) topn_offer(list, thr, lists[w2][lane], n, lane, KeyDescending());
    if (lane < n) {
        types[(int64_t)k * n + lane] = list ? (int32_t)(uint32_t)list : -1;              // unfilled slots: -1 / 0
        counts[(int64_t)k * n + lane] = (int32_t)(list >> 32);
    }
    if (lane == 0) nonzero[k] = nzs[0] + nzs[1] + nzs[2] + nzs[3];                      // sortedWords.size()
}

// ---------------------------------------------------------------------------------------------------------------
// collectDocumentStatistics DIAG:158-235 over view 0, one wave per entity (static: wave g takes entities g, g + G, ...).
// Per wave in LDS: the entity's topic counts cnt[K], the list of its distinct topics, and per topic the mask of the top-N positions
// whose type occurs with that topic (bit i: position i "supported", DIAG:175-177,210); all three are cleared entry by entry when the
// entity is done.  c log c goes to a per-wave fp64 row (acc[K]) that is written out once: partial[g][k].  The per-topic integer
// counters sit in LDS per block when they fit (flushed with one atomic per non-zero counter), else in global memory; the co-document
// matrices take global int atomics.
struct DiagDocArgs {
    const int64_t* doc_off; const int32_t* tok; const int32_t* z;
    int64_t D; int K, V, N;
    double g_alpha0_base;                  // gamma[0] * alphaSum[0], the denominator's first term (DIAG:198)
    double gamma0; const double* alpha0;   // alpha[0][0..K)
    const int32_t* tl_types;               // [K][N] each topic's real top types in ascending type order
    const int8_t* tl_pos;                  //   and their positions in the top-N list
    const int32_t* tl_n;                   // [K] real top words = min(N, nonzero)
    const int8_t* pos0;                    // [K] position of type 0 among the real top words, -1 none (the padding quirk)
    int32_t* g_ctr;                        // [K][2 + 7] non-zero documents, rank-1 documents, documents at the proportions
    int32_t* codoc;                        // [K][N][N]
    double* partial;                       // [G][K]
    unsigned long long* tokens;            // numTokens
    int32_t* err;                          // set when a token Java's pass would throw on (DIAG:171,173)
    int wpb, lds_ctr;
};

constexpr int NCTR = 2 + DIAG_NPROP;
__host__ __device__ inline size_t diag_ctr_bytes(int K) { return ((size_t)K * NCTR * 4 + 15) & ~(size_t)15; }   // (keeps the waves' fp64 rows aligned)

__global__ __launch_bounds__(256) void diag_doc_kernel(DiagDocArgs a)
{
    extern __shared__ unsigned char diag_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = a.K, N = a.N;
    int32_t* lctr = (int32_t*)diag_lds;                                            // [K][NCTR] when a.lds_ctr
    unsigned char* wbase = diag_lds + (a.lds_ctr ? diag_ctr_bytes(K) : 0);
    const size_t per_wave = (size_t)K * (8 + 8 + 4 + 4) + 16;
    unsigned char* mine = wbase + (size_t)wave * per_wave;
    double* acc = (double*)mine;
    unsigned long long* mask = (unsigned long long*)(mine + (size_t)K * 8);
    int32_t* cnt = (int32_t*)(mine + (size_t)K * 16);
    int32_t* list = (int32_t*)(mine + (size_t)K * 20);
    int32_t* nlist = (int32_t*)(mine + (size_t)K * 24);
    int32_t* ctr = a.lds_ctr ? lctr : a.g_ctr;
    if (a.lds_ctr) for (int i = threadIdx.x; i < K * NCTR; i += blockDim.x) lctr[i] = 0;
    for (int k = lane; k < K; k += WAVE) { acc[k] = 0.0; mask[k] = 0; cnt[k] = 0; }
    if (lane == 0) *nlist = 0;
    __syncthreads();
    const int64_t G = (int64_t)gridDim.x * a.wpb, gw = (int64_t)blockIdx.x * a.wpb + wave;
    const uint64_t all_n = N == 64 ? ~0ull : ((1ull << N) - 1);
    unsigned long long ntok = 0;
    int bad = 0;
    for (int64_t d = gw; d < a.D; d += G) {
        const int64_t b = a.doc_off[d], e = a.doc_off[d + 1];
        const int len = (int)(e - b);
        if (len <= 0) continue;                                                     // DIAG:182 (and an absent view: no tokens)
        ntok += len;                                                                // DIAG:170
        for (int64_t i = b + lane; i < e; i += WAVE) {
            const int t = a.tok[i], zz = a.z[i];
            if (zz < 0 || zz >= K || t < 0 || t >= a.V) { bad = 1; continue; }
            if (atomicAdd(&cnt[zz], 1) == 0) list[atomicAdd(nlist, 1)] = zz;        // DIAG:173
            const int nr = a.tl_n[zz];
            const int32_t* ty = a.tl_types + (int64_t)zz * N;
            int lo = 0, hi = nr;                                                    // DIAG:175: is `t` one of the topic's top words?
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ty[mid] < t) lo = mid + 1; else hi = mid; }
            if (lo < nr && ty[lo] == t) atomicOr(&mask[zz], 1ull << a.tl_pos[(int64_t)zz * N + lo]);
        }
        LDS_FENCE();
        const int nl = *nlist;
        const double denom = a.g_alpha0_base + len;                                 // (double) gamma[0] * alphaSum[0] + docLength
        unsigned long long best = 0;
        for (int s = lane; s < nl; s += WAVE) {
            const int k = list[s], c = cnt[k];
            int32_t* ck = ctr + (int64_t)k * NCTR;
            atomicAdd(&ck[0], 1);                                                   // DIAG:189
            const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(K - 1 - k);
            if (key > best) best = key;                                             // DIAG:191-194: strict >, ascending topics
            acc[k] += (double)c * log((double)c);                                   // DIAG:196
            const double prop = (a.gamma0 * a.alpha0[k] + c) / denom;               // DIAG:198
            for (int i = 0; i < DIAG_NPROP; i++) {                                  // DIAG:199-204
                if (prop < c_doc_proportions[i]) break;
                atomicAdd(&ck[2 + i], 1);
            }
            uint64_t pm = mask[k];
            const int nr = a.tl_n[k], p0 = a.pos0[k];
            if (nr < N && p0 >= 0 && ((pm >> p0) & 1ull)) pm |= all_n & ~((1ull << nr) - 1);   // DIAG:146-150,207-220: padding holds type 0
            int32_t* cm = a.codoc + (int64_t)k * N * N;
            for (uint64_t r = pm; r; r &= r - 1) {                                  // DIAG:209-221
                const int i = __ffsll((long long)r) - 1;
                atomicAdd(&cm[i * N + i], 1);
                for (uint64_t q = r & (r - 1); q; q &= q - 1) {
                    const int j = __ffsll((long long)q) - 1;
                    atomicAdd(&cm[i * N + j], 1);
                    atomicAdd(&cm[j * N + i], 1);
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const unsigned long long x = __shfl_xor(best, o, WAVE); if (x > best) best = x; }
        if (lane == 0) atomicAdd(&ctr[(int64_t)(K - 1 - (int)(uint32_t)best) * NCTR + 1], 1);   // DIAG:228-230
        LDS_FENCE();
        for (int s = lane; s < nl; s += WAVE) { const int k = list[s]; cnt[k] = 0; mask[k] = 0; }   // DIAG:223-224
        if (lane == 0) *nlist = 0;
        LDS_FENCE();
    }
    if (__builtin_amdgcn_ballot_w64(bad != 0) && lane == 0) atomicOr(a.err, 1);
    if (lane == 0 && ntok) atomicAdd(a.tokens, ntok);
    double* out = a.partial + gw * K;
    for (int k = lane; k < K; k += WAVE) out[k] = acc[k];
    if (a.lds_ctr) {
        __syncthreads();
        for (int i = threadIdx.x; i < K * NCTR; i += blockDim.x) if (lctr[i]) atomicAdd(&a.g_ctr[i], lctr[i]);
    }
}

__global__ __launch_bounds__(256) void diag_sum_partials(const double* __restrict__ partial, int G, int K, double* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int g = 0; g < G; g++) s += partial[(int64_t)g * K + k];
    out[k] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// Column sums over topic k's words of view 0 (every type with n_wk > 0, which is the TreeSet's content), T = tokensPerTopic[0][k]:
//   [0] sum (c/T) log(c V_0 / T)                 uniform_dist DIAG:280-287     [1] the same over |term|
//   [2] sum (c/T) log((numTokens/T) c / wtc[w])  corpus_dist  DIAG:377-395     [3] the same over |term|
//   [4] sum (c/T)^2                               eff_num_words DIAG:352-357
//   [5] sum tw[w] c                               calcDiscrWeightWithinTopics PTM:2250-2255 (totalTopicCnts)
//   [6] sum (tw[w] c / [5])^2                     PTM:2258-2262
// Each thread's share in ascending type order, then a fixed-order tree over the block.
__device__ __forceinline__ double block_sum(double v, double* red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void diag_columns_kernel(const int32_t* __restrict__ nkw, int V, const int32_t* __restrict__ nk,
                                                           const int64_t* __restrict__ wtc, double num_tokens, const double* __restrict__ tw,
                                                           double* __restrict__ out)
{
    __shared__ double red[256];
    const int k = blockIdx.x;
    const int32_t* col = nkw + (int64_t)k * V;
    const int T = nk[k];
    const double coef = num_tokens / T;
    double su = 0, au = 0, sc = 0, ac = 0, se = 0, sd = 0;
    for (int w = threadIdx.x; w < V; w += blockDim.x) {
        const int c = col[w];
        if (c <= 0) continue;
        const double cd = (double)c;
        const double p = cd / T;
        const double u = p * log((cd * V) / T);
        const double q = p * log(coef * cd / (double)wtc[w]);
        su += u; au += fabs(u); sc += q; ac += fabs(q);
        se += p * p;
        sd += tw[w] * cd;
    }
    double r[NCOL];
    r[0] = block_sum(su, red); r[1] = block_sum(au, red); r[2] = block_sum(sc, red); r[3] = block_sum(ac, red);
    r[4] = block_sum(se, red); r[5] = block_sum(sd, red);
    const double total = r[5];
    double s2 = 0;
    for (int w = threadIdx.x; w < V; w += blockDim.x) {
        const int c = col[w];
        if (c <= 0) continue;
        const double pr = tw[w] * (double)c / total;
        s2 += pr * pr;
    }
    r[6] = block_sum(s2, red);
    if (threadIdx.x == 0) for (int i = 0; i < NCOL; i++) out[(int64_t)k * NCOL + i] = r[i];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int diag_ready(mvhdp_ctx* h, bool need_hyper)
{
    for (int m = 0; m < h->mm.M; m++)
        if (!h->have_corpus[m]) FAIL(h, MVHDP_ERR_STATE, "diagnostics: set_corpus has not been called for every view");
    if (int rc = require_current_counts(h, "diagnostics")) return rc;
    if (need_hyper && !h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "diagnostics before set_hyper");
    return MVHDP_OK;
}

// the transposed n_wk of view m in a fresh device buffer
hipError_t transpose_view(mvhdp_ctx* h, int m, DevArray<int32_t>& nkw)
{
    const MvModel& mm = h->mm;
    hipError_t e = nkw.alloc((size_t)mm.V[m] * mm.K);
    if (e != hipSuccess || mm.V[m] == 0) return e;
    dim3 grid((mm.V[m] + 63) / 64, (mm.K + 63) / 64);
    hipLaunchKernelGGL(diag_transpose_kernel, grid, dim3(256), 0, h->stream, mm.counts + mm.rowbase[m] * mm.K, mm.V[m], mm.K, nkw.get());
    return hipGetLastError();
}

hipError_t launch_topn(mvhdp_ctx* h, const int32_t* nkw, int m, int n, int32_t* types, int32_t* counts, int32_t* nonzero)
{
    hipLaunchKernelGGL(diag_topn_kernel, dim3(h->mm.K), dim3(256), 0, h->stream, nkw, h->mm.V[m], n, types, counts, nonzero);
    return hipGetLastError();
}

// PTM:2193-2226 over every view: per_view[m] (the running mean, accumulators not reset between views, nonZeroSkewCnt from 1);
// tw_dev / rowsum_dev (device, [V_m] each) receive view `want`'s per-type weights and row sums when not null.
int discr_weights_device(mvhdp_ctx* h, double* per_view, int want, double* tw_dev, int64_t* rowsum_dev)
{
    const MvModel& mm = h->mm;
    DevArray<double> d_tw, d_ps;
    DevArray<int64_t> d_rs;
    DevArray<long long> d_pc;
    int64_t vmax = 0;
    for (int m = 0; m < mm.M; m++) vmax = std::max<int64_t>(vmax, mm.V[m]);
    HIPC(h, d_tw.alloc((size_t)vmax));
    HIPC(h, d_rs.alloc((size_t)vmax));
    HIPC(h, d_ps.alloc((size_t)mm.M * ROWS_BLOCKS));
    HIPC(h, d_pc.alloc((size_t)mm.M * ROWS_BLOCKS));
    for (int m = 0; m < mm.M; m++) {
        const bool mine = m == want && tw_dev;
        double* twm = mine ? tw_dev : d_tw.get();
        int64_t* rsm = mine && rowsum_dev ? rowsum_dev : d_rs.get();
        if (mm.V[m] > 0)
            LAUNCH(h, diag_rows_kernel, dim3(ROWS_BLOCKS), dim3(256), 0, h->stream, mm.counts + mm.rowbase[m] * mm.K, mm.V[m], mm.K,
                   twm, rsm, d_ps + (size_t)m * ROWS_BLOCKS, d_pc + (size_t)m * ROWS_BLOCKS);
        else {                                                                 // a part of each array: the byte counts by hand
            HIPC(h, hipMemsetAsync(d_ps + (size_t)m * ROWS_BLOCKS, 0, ROWS_BLOCKS * sizeof(double), h->stream));
            HIPC(h, hipMemsetAsync(d_pc + (size_t)m * ROWS_BLOCKS, 0, ROWS_BLOCKS * sizeof(long long), h->stream));
        }
    }
    std::vector<double> ps((size_t)mm.M * ROWS_BLOCKS);
    std::vector<long long> pc((size_t)mm.M * ROWS_BLOCKS);
    HIPC(h, d_ps.download(ps.data(), ps.size(), h->stream));
    HIPC(h, d_pc.download(pc.data(), pc.size(), h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    double skewSum = 0;                                                    // PTM:2190-2191
    long long nonZeroSkewCnt = 1;
    for (int m = 0; m < mm.M; m++) {
        for (int i = 0; i < ROWS_BLOCKS; i++) { skewSum += ps[(size_t)m * ROWS_BLOCKS + i]; nonZeroSkewCnt += pc[(size_t)m * ROWS_BLOCKS + i]; }
        if (per_view) per_view[m] = skewSum / (double)nonZeroSkewCnt;    // PTM:2223
    }
    return MVHDP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// pieces a group composes (declared in mvhdp_ctx.h)
// ---------------------------------------------------------------------------------------------------------------
int mvhdp_diag_model(mvhdp_ctx* h, int N, DiagModel& dm)
{
    int rc = diag_ready(h, true); if (rc) return rc;
    MvModel& mm = h->mm;
    const int K = mm.K, V0 = mm.V[0];
    HIPC(h, hipSetDevice(h->device));
    DevArray<int32_t> nkw, d_types, d_counts, d_nz;
    DevArray<double> d_tw;
    DevArray<int64_t> d_rs;
    HIPC(h, transpose_view(h, 0, nkw));
    HIPC(h, d_types.alloc((size_t)K * N)); HIPC(h, d_counts.alloc((size_t)K * N)); HIPC(h, d_nz.alloc((size_t)K));
    HIPC(h, d_tw.alloc((size_t)V0)); HIPC(h, d_rs.alloc((size_t)V0));
    HIPC(h, launch_topn(h, nkw, 0, N, d_types, d_counts, d_nz));
    dm.N = N;
    dm.per_view.assign((size_t)mm.M, 0.0);
    rc = discr_weights_device(h, dm.per_view.data(), 0, d_tw, d_rs); if (rc) return rc;
    dm.types.resize((size_t)K * N); dm.counts.resize((size_t)K * N); dm.nonzero.resize((size_t)K);
    dm.word_type_counts.resize((size_t)V0); dm.type_weight.resize((size_t)V0);
    dm.nk.resize((size_t)K);
    HIPC(h, d_types.download(dm.types.data(), dm.types.size(), h->stream));
    HIPC(h, d_counts.download(dm.counts.data(), dm.counts.size(), h->stream));
    HIPC(h, d_nz.download(dm.nonzero.data(), dm.nonzero.size(), h->stream));
    HIPC(h, d_rs.download(dm.word_type_counts.data(), (size_t)V0, h->stream));
    HIPC(h, d_tw.download(dm.type_weight.data(), (size_t)V0, h->stream));
    HIPC(h, hipMemcpyAsync(dm.nk.data(), mm.counts + mm.rowbase[mm.M] * K, (size_t)K * 4, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

int mvhdp_diag_docs(mvhdp_ctx* h, const DiagModel& dm, DiagAcc& acc)
{
    int rc = diag_ready(h, true); if (rc) return rc;
    MvModel& mm = h->mm;
    const int K = mm.K, N = dm.N;
    if (acc.codoc.empty()) acc.reset(K, N);
    if (mm.D == 0) return MVHDP_OK;
    HIPC(h, hipSetDevice(h->device));
    // every topic's real top words in ascending type order, with their positions (the doc kernel's lookup)
    std::vector<int32_t> tl_types((size_t)K * N, INT32_MAX), tl_n((size_t)K);
    std::vector<int8_t> tl_pos((size_t)K * N, 0), pos0((size_t)K, -1);
    for (int k = 0; k < K; k++) {
        const int nr = std::min(N, dm.nonzero[k]);
        tl_n[k] = nr;
        std::vector<std::pair<int32_t, int>> v;
        for (int i = 0; i < nr; i++) { v.emplace_back(dm.types[(size_t)k * N + i], i); if (dm.types[(size_t)k * N + i] == 0) pos0[k] = (int8_t)i; }
        std::sort(v.begin(), v.end());
        for (int i = 0; i < nr; i++) { tl_types[(size_t)k * N + i] = v[i].first; tl_pos[(size_t)k * N + i] = (int8_t)v[i].second; }
    }
    const size_t per_wave = (size_t)K * 24 + 16;
    int wpb = 4;
    while (wpb > 1 && wpb * per_wave > 65536) wpb >>= 1;
    if (per_wave > 65536) FAIL(h, MVHDP_ERR_UNSUPPORTED, "diagnostics: too many topics for the document pass");
    const bool lds_ctr = diag_ctr_bytes(K) + wpb * per_wave <= 65536;
    const size_t lds = (lds_ctr ? diag_ctr_bytes(K) : 0) + wpb * per_wave;
    const int64_t blocks = (mm.D + wpb - 1) / wpb;
    const int grid = (int)std::min<int64_t>(blocks, DOC_WAVES / wpb);
    const int G = grid * wpb;
    DevArray<int32_t> d_tlt, d_tln, d_ctr, d_codoc, d_err;
    DevArray<int8_t> d_tlp, d_pos0;
    DevArray<double> d_part, d_scl;
    DevArray<unsigned long long> d_tok;
    HIPC(h, d_tlt.alloc(tl_types.size())); HIPC(h, d_tln.alloc(tl_n.size())); HIPC(h, d_tlp.alloc(tl_pos.size())); HIPC(h, d_pos0.alloc(pos0.size()));
    HIPC(h, d_ctr.alloc((size_t)K * NCTR)); HIPC(h, d_codoc.alloc((size_t)K * N * N)); HIPC(h, d_err.alloc(1));
    HIPC(h, d_part.alloc((size_t)G * K)); HIPC(h, d_scl.alloc((size_t)K)); HIPC(h, d_tok.alloc(1));
    const hipStream_t s = h->stream;
    HIPC(h, d_tlt.upload(tl_types.data(), tl_types.size(), s));
    HIPC(h, d_tln.upload(tl_n.data(), tl_n.size(), s));
    HIPC(h, d_tlp.upload(tl_pos.data(), tl_pos.size(), s));
    HIPC(h, d_pos0.upload(pos0.data(), pos0.size(), s));
    HIPC(h, d_ctr.fill(0, s));
    HIPC(h, d_codoc.fill(0, s));
    HIPC(h, d_err.fill(0, s));
    HIPC(h, d_tok.fill(0, s));
    DiagDocArgs a{};
    a.doc_off = mm.doc_off[0]; a.tok = mm.tok[0]; a.z = mm.z[0];
    a.D = mm.D; a.K = K; a.V = mm.V[0]; a.N = N;
    a.gamma0 = mm.gamma[0]; a.g_alpha0_base = (double)mm.gamma[0] * mm.alpha_sum[0]; a.alpha0 = mm.alpha;
    a.tl_types = d_tlt; a.tl_pos = d_tlp; a.tl_n = d_tln; a.pos0 = d_pos0;
    a.g_ctr = d_ctr; a.codoc = d_codoc; a.partial = d_part; a.tokens = d_tok; a.err = d_err;
    a.wpb = wpb; a.lds_ctr = lds_ctr ? 1 : 0;
    HIPC(h, hipFuncSetAttribute((const void*)diag_doc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LAUNCH(h, diag_doc_kernel, dim3(grid), dim3(64 * wpb), lds, s, a);
    LAUNCH(h, diag_sum_partials, dim3((K + 255) / 256), dim3(256), 0, s, d_part, G, K, d_scl);
    std::vector<int32_t> ctr((size_t)K * NCTR), codoc((size_t)K * N * N);
    std::vector<double> scl((size_t)K);
    int32_t err = 0;
    unsigned long long ntok = 0;
    HIPC(h, d_ctr.download(ctr.data(), ctr.size(), s));
    HIPC(h, d_codoc.download(codoc.data(), codoc.size(), s));
    HIPC(h, d_scl.download(scl.data(), scl.size(), s));
    HIPC(h, d_err.download(&err, 1, s));
    HIPC(h, d_tok.download(&ntok, 1, s));
    HIPC(h, hipStreamSynchronize(s));
    if (err) FAIL(h, MVHDP_ERR_STATE, "diagnostics: a view-0 token is unassigned or out of vocabulary (collectDocumentStatistics would throw, DIAG:171-173)");
    for (int k = 0; k < K; k++) {
        acc.nonzero_docs[k] += ctr[(size_t)k * NCTR];
        acc.rank1_docs[k] += ctr[(size_t)k * NCTR + 1];
        for (int i = 0; i < DIAG_NPROP; i++) acc.at_proportions[(size_t)k * DIAG_NPROP + i] += ctr[(size_t)k * NCTR + 2 + i];
        acc.sum_count_log_count[k] += scl[k];
    }
    for (size_t i = 0; i < codoc.size(); i++) acc.codoc[i] += codoc[i];
    acc.num_tokens += (int64_t)ntok;
    return MVHDP_OK;
}

// The column reductions (on h) and the thirteen rows of DIAG:104-116; `out` is written only when everything has succeeded.
int mvhdp_diag_finish(mvhdp_ctx* h, const DiagModel& dm, const DiagAcc& acc, const mvhdp_diag_args* args, const mvhdp_diag_out* out)
{
    MvModel& mm = h->mm;
    const int K = mm.K, N = dm.N, V0 = mm.V[0];
    int64_t nk_total = 0;
    for (int k = 0; k < K; k++) nk_total += dm.nk[k];
    if (nk_total != acc.num_tokens)
        FAIL(h, MVHDP_ERR_STATE, "diagnostics: tokensPerTopic[0] does not add up to the view-0 tokens (counts not current)");
    HIPC(h, hipSetDevice(h->device));
    std::vector<double> col((size_t)K * NCOL);
    {
        DevArray<int32_t> nkw, d_nk;
        DevArray<int64_t> d_wtc;
        DevArray<double> d_tw, d_col;
        HIPC(h, transpose_view(h, 0, nkw));
        HIPC(h, d_nk.alloc((size_t)K)); HIPC(h, d_wtc.alloc((size_t)V0)); HIPC(h, d_tw.alloc((size_t)V0)); HIPC(h, d_col.alloc(col.size()));
        HIPC(h, d_nk.upload(dm.nk.data(), (size_t)K, h->stream));
        HIPC(h, d_wtc.upload(dm.word_type_counts.data(), (size_t)V0, h->stream));
        HIPC(h, d_tw.upload(dm.type_weight.data(), (size_t)V0, h->stream));
        LAUNCH(h, diag_columns_kernel, dim3(K), dim3(256), 0, h->stream, nkw, V0, d_nk, d_wtc, (double)acc.num_tokens, d_tw, d_col);
        HIPC(h, d_col.download(col.data(), col.size(), h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> sc((size_t)MVHDP_DIAG_ROWS * K, 0.0), ws((size_t)MVHDP_DIAG_ROWS * K * N, 0.0);
    auto S = [&](int row, int k) -> double& { return sc[(size_t)row * K + k]; };
    auto W = [&](int row, int k, int i) -> double& { return ws[((size_t)row * K + k) * N + i]; };
    const double* alpha0 = h->h_alpha.data();                       // [0][0..K]
    double avgAlpha = 0;                                            // DIAG:315-325
    int acnt = 0;
    for (int kk = 0; kk <= K; kk++) { avgAlpha += alpha0[kk]; acnt += alpha0[kk] == 0 ? 0 : 1; }
    avgAlpha = avgAlpha / acnt;
    const double beta0 = mm.beta[0];
    for (int k = 0; k < K; k++) {
        const int T = dm.nk[k];
        const int nr = std::min(N, dm.nonzero[k]);
        const int32_t* cm = acc.codoc.data() + (size_t)k * N * N;
        const double* c = col.data() + (size_t)k * NCOL;
        S(MVHDP_DIAG_TOKENS, k) = T;                                                                  // DIAG:242-250
        S(MVHDP_DIAG_DOCUMENT_ENTROPY, k) = -acc.sum_count_log_count[k] / T + std::log((double)T);    // DIAG:256
        if (args->word_length) {                                                                      // DIAG:462-483
            int total = 0;
            for (int i = 0; i < nr; i++) { const int len = args->word_length[dm.types[(size_t)k * N + i]]; total += len; W(MVHDP_DIAG_WORD_LENGTH, k, i) = len; }
            S(MVHDP_DIAG_WORD_LENGTH, k) = (double)total / N;
        } else {
            S(MVHDP_DIAG_WORD_LENGTH, k) = nan;
            for (int i = 0; i < N; i++) W(MVHDP_DIAG_WORD_LENGTH, k, i) = nan;
        }
        double topicScore = 0.0;                                                                      // DIAG:544-570
        for (int row = 0; row < N; row++) {
            double rowScore = 0.0, minScore = 0.0;
            for (int cc = 0; cc < row; cc++) {
                const double score = std::log((cm[row * N + cc] + beta0) / (cm[cc * N + cc] + beta0));
                rowScore += score;
                if (score < minScore) minScore = score;
            }
            topicScore += rowScore;
            W(MVHDP_DIAG_COHERENCE, k, row) = minScore;
        }
        S(MVHDP_DIAG_COHERENCE, k) = topicScore;
        const double tdw = c[5] == 0 ? 0.0 : c[6];                                                    // PTM:2243-2262 (no word: 0)
        if (alpha0[k] != 0) {                                                                         // DIAG:297-338
            const double diffLogWeight = std::fabs(std::log10(alpha0[k]) - std::log10(avgAlpha));
            S(MVHDP_DIAG_NORM_DISCR_WEIGHT, k) = tdw / diffLogWeight;
            S(MVHDP_DIAG_DISCR_WEIGHT, k) = tdw;
        }
        S(MVHDP_DIAG_UNIFORM_DIST, k) = c[0];                                                         // DIAG:262-295
        S(MVHDP_DIAG_CORPUS_DIST, k) = c[2];                                                          // DIAG:368-404
        const double coefficient = (double)acc.num_tokens / T;
        for (int i = 0; i < nr; i++) {
            const double cnt = dm.counts[(size_t)k * N + i];
            const int type = dm.types[(size_t)k * N + i];
            W(MVHDP_DIAG_UNIFORM_DIST, k, i) = (cnt / T) * std::log((cnt * V0) / T);
            W(MVHDP_DIAG_CORPUS_DIST, k, i) = (cnt / T) * std::log(coefficient * cnt / (double)dm.word_type_counts[type]);
        }
        S(MVHDP_DIAG_EFF_NUM_WORDS, k) = 1.0 / c[4];                                                  // DIAG:340-363
        {                                                                                             // DIAG:406-457
            std::vector<double> wd((size_t)N, 0.0), dd((size_t)N, 0.0);
            double wordSum = 0.0, docSum = 0.0;
            for (int i = 0; i < nr; i++) { wd[i] = dm.counts[(size_t)k * N + i]; dd[i] = cm[i * N + i]; wordSum += wd[i]; docSum += dd[i]; }
            double ts = 0.0;
            for (int i = 0; i < N; i++) {
                const double p = wd[i] / wordSum, q = dd[i] / docSum, meanProb = 0.5 * (p + q);
                double score = 0.0;
                if (p > 0) score += 0.5 * p * std::log(p / meanProb);
                if (q > 0) score += 0.5 * q * std::log(q / meanProb);
                W(MVHDP_DIAG_TOKEN_DOC_DIFF, k, i) = score;
                ts += score;
            }
            S(MVHDP_DIAG_TOKEN_DOC_DIFF, k) = ts;
        }
        const int32_t* ap = acc.at_proportions.data() + (size_t)k * DIAG_NPROP;
        S(MVHDP_DIAG_RANK_1_DOCS, k) = (double)acc.rank1_docs[k] / acc.nonzero_docs[k];             // DIAG:573-581
        S(MVHDP_DIAG_ALLOCATION_RATIO, k) = (double)ap[6] / ap[1];                                   // DIAG:583-598 (FIFTY / TWO percent)
        S(MVHDP_DIAG_ALLOCATION_COUNT, k) = (double)ap[5] / acc.nonzero_docs[k];                     // DIAG:600-613
    }
    // everything is known: now the caller's arrays
    std::copy(sc.begin(), sc.end(), out->scores);
    if (out->word_scores) std::copy(ws.begin(), ws.end(), out->word_scores);
    if (out->codoc) std::copy(acc.codoc.begin(), acc.codoc.end(), out->codoc);
    if (out->top_types) std::copy(dm.types.begin(), dm.types.end(), out->top_types);
    if (out->top_counts) std::copy(dm.counts.begin(), dm.counts.end(), out->top_counts);
    if (out->nonzero) std::copy(dm.nonzero.begin(), dm.nonzero.end(), out->nonzero);
    if (out->num_rank1_docs) std::copy(acc.rank1_docs.begin(), acc.rank1_docs.end(), out->num_rank1_docs);
    if (out->num_nonzero_docs) std::copy(acc.nonzero_docs.begin(), acc.nonzero_docs.end(), out->num_nonzero_docs);
    if (out->num_docs_at_proportions) std::copy(acc.at_proportions.begin(), acc.at_proportions.end(), out->num_docs_at_proportions);
    if (out->sum_count_log_count) std::copy(acc.sum_count_log_count.begin(), acc.sum_count_log_count.end(), out->sum_count_log_count);
    if (out->word_type_counts) for (int w = 0; w < V0; w++) out->word_type_counts[w] = (int32_t)dm.word_type_counts[w];
    if (out->num_tokens) *out->num_tokens = acc.num_tokens;
    if (out->discr_weight_per_view) std::copy(dm.per_view.begin(), dm.per_view.end(), out->discr_weight_per_view);
    return MVHDP_OK;
}

int mvhdp_diag_check_args(mvhdp_ctx* h, const mvhdp_diag_args* args, const mvhdp_diag_out* out)
{
    if (!args || !out) FAIL(h, MVHDP_ERR_INVALID_ARG, "diagnostics: null args or out");
    if (args->num_top_words < 1 || args->num_top_words > MVHDP_DIAG_MAX_TOP_WORDS) FAIL(h, MVHDP_ERR_INVALID_ARG, "diagnostics: num_top_words must be 1..64");
    if (!out->scores) FAIL(h, MVHDP_ERR_INVALID_ARG, "diagnostics: out->scores is null");
    if (h->mm.K > 32767) FAIL(h, MVHDP_ERR_INVALID_ARG, "diagnostics: too many topics");
    return MVHDP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the C ABI of one handle
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mvhdp_top_words(mvhdp_handle h, int32_t m, int32_t n, int32_t* types, int32_t* counts, int32_t* nonzero)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "top_words: bad view");
    if (n < 1 || n > MVHDP_DIAG_MAX_TOP_WORDS) FAIL(h, MVHDP_ERR_INVALID_ARG, "top_words: n must be 1..64");
    if (!types || !counts || !nonzero) FAIL(h, MVHDP_ERR_INVALID_ARG, "top_words: null output");
    int rc = diag_ready(h, false); if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const int K = mm.K;
    DevArray<int32_t> nkw, d_t, d_c, d_nz;
    HIPC(h, transpose_view(h, m, nkw));
    HIPC(h, d_t.alloc((size_t)K * n)); HIPC(h, d_c.alloc((size_t)K * n)); HIPC(h, d_nz.alloc((size_t)K));
    HIPC(h, launch_topn(h, nkw, m, n, d_t, d_c, d_nz));
    std::vector<int32_t> t((size_t)K * n), c((size_t)K * n), z((size_t)K);
    HIPC(h, d_t.download(t.data(), t.size(), h->stream));
    HIPC(h, d_c.download(c.data(), c.size(), h->stream));
    HIPC(h, d_nz.download(z.data(), z.size(), h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::copy(t.begin(), t.end(), types); std::copy(c.begin(), c.end(), counts); std::copy(z.begin(), z.end(), nonzero);
    return MVHDP_OK;
}

extern "C" int mvhdp_discr_weights(mvhdp_handle h, double* per_view, int32_t m, double* type_weight)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (!per_view) FAIL(h, MVHDP_ERR_INVALID_ARG, "discr_weights: per_view is null");
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "discr_weights: bad view");
    int rc = diag_ready(h, false); if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    DevArray<double> d_tw;
    if (type_weight) HIPC(h, d_tw.alloc((size_t)mm.V[m]));
    std::vector<double> pv((size_t)mm.M), tw(type_weight ? (size_t)mm.V[m] : 0);
    rc = discr_weights_device(h, pv.data(), m, d_tw, nullptr); if (rc) return rc;
    if (type_weight && mm.V[m] > 0) {
        HIPC(h, d_tw.download(tw.data(), tw.size(), h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        std::copy(tw.begin(), tw.end(), type_weight);
    }
    std::copy(pv.begin(), pv.end(), per_view);
    return MVHDP_OK;
}

extern "C" int mvhdp_diagnostics(mvhdp_handle h, const mvhdp_diag_args* args, mvhdp_diag_out* out)
{
    CHECK_H(h);
    int rc = mvhdp_diag_check_args(h, args, out); if (rc) return rc;
    DiagModel dm;
    rc = mvhdp_diag_model(h, args->num_top_words, dm); if (rc) return rc;
    DiagAcc acc;
    acc.reset(h->mm.K, dm.N);
    rc = mvhdp_diag_docs(h, dm, acc); if (rc) return rc;
    return mvhdp_diag_finish(h, dm, acc, args, out);
}
