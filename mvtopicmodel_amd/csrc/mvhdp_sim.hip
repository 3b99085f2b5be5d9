// mvhdp_sim.hip — what SciTopicFlow does with a trained model (FLOW:246-260), on the device (include/mvhdp.h has the contracts):
//   sim_prepare_kernel      per row: entries <= min_weight zeroed, |row| = sqrt of the fp64 chain of squares, the row's class
//   sim_normalise_kernel    row / |row| in fp64, stored as fp32 into a zero-padded image
//   sim_screen_kernel       the screen: 128 x 128 tiles of X X^T on v_mfma_f32_32x32x2_f32, candidates appended by wave
//   sim_exact_kernel        every candidate recomputed by the reference's fp64 chain and tested
//   sim_jsd_kernel          Maths.jensenShannonDivergence per pair, fp64 VALU, no screen
//   top_count_kernel / top_fill_kernel / group_sum_kernel
//                           the thresholded topic lists of saveTopicsPerDoc (PTM:2890-2926) and their sums per group (FLOW:807-1083):
//                           one wave per entity or group, lanes over topics, kept flags from a rank among the weights >= threshold
// No floating-point atomics: every fp64 sum is a chain in a fixed order.  The integer appends (candidates, survivors) are unordered;
// the host sorts each stripe's survivors by (i << 32) | j.
#include "mvhdp_screen.h"
#include "mvhdp_select.h"
#include "mvhdp_side.h"

namespace {

constexpr int WV = 64;

// ---------------------------------------------------------------------------------------------------------------
// One thread per row.  x is cleaned in place.
__global__ __launch_bounds__(256) void sim_prepare_kernel(double* __restrict__ x, int n, int dim, double min_weight, double* __restrict__ norm, uint8_t* __restrict__ cls)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double* row = x + (int64_t)r * dim;
    const double lo = 0x1p-500, hi = 0x1p500;
    double s = 0.0;
    bool wild = false;
    for (int k = 0; k < dim; k++) {
        double v = row[k];
        if (v <= min_weight) { v = 0.0; row[k] = 0.0; }
        s = s + v * v;                                         // SparseVector.twoNorm: dmul, dadd, ascending
        const double a = fabs(v);
        wild = wild || (v != 0.0 && !(a >= lo && a <= hi));
    }
    const double nr = sqrt(s);
    norm[r] = nr;
    cls[r] = !(nr > 0.0 && nr < INFINITY) ? ROW_OUT : wild ? ROW_WILD : ROW_TAME;
}

// xn: [n_pad][ld] fp32, zero beyond (n, dim) and for rows that are not ROW_TAME
__global__ __launch_bounds__(256) void sim_normalise_kernel(const double* __restrict__ x, const double* __restrict__ norm, const uint8_t* __restrict__ cls,
                                                            int n, int dim, int64_t ld, float* __restrict__ xn)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * dim) return;
    const int r = (int)(i / dim), k = (int)(i - (int64_t)r * dim);
    xn[(int64_t)r * ld + k] = cls[r] == ROW_TAME ? (float)(x[i] / norm[r]) : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------
// The screen.  Block (b, a) of the stripe that starts at row r0 computes the 128 x 128 cells rows r0 + 128 a .., columns r0 + 128 b ..
// (b >= a only) with screen_tile (mvhdp_screen.h has the layout); xn is padded with zero rows to r0 + 128 * tiles.
__global__ __launch_bounds__(256) void sim_screen_kernel(const float* __restrict__ xn, int64_t ld, int kslabs, const uint8_t* __restrict__ cls,
                                                         int n, int r0, int r1, double cut, u64* __restrict__ cand, u64 cap, u64* counter)
{
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (tb < ta) return;
    __shared__ __attribute__((aligned(16))) float As[SCREEN_TILE * SCREEN_LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[SCREEN_TILE * SCREEN_LDS_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64, lr = lane & 31, lh = lane >> 5;
    const int64_t arow0 = (int64_t)r0 + (int64_t)ta * SCREEN_TILE, brow0 = (int64_t)r0 + (int64_t)tb * SCREEN_TILE;
    f32x16 acc[2][2];
    screen_tile(xn, xn, ld, kslabs, arow0, brow0, As, Bs, acc);

    // epilogue: cell (i, j) is a candidate when i < j, both rows can pair, and either one is not screened or screen > threshold - margin.
    // Two passes over the accumulators: the block counts its candidates, takes its room with ONE atomic (a wave-level atomic per ballot
    // on the one counter serialises the whole grid: 452 ms instead of 42 at n = 100 000, profiles/similarity.md), then writes.
    const int64_t jb = brow0 + wc + lr;                        // + 32 b
    const int64_t ib = arow0 + wr + 4 * lh;                    // + 32 a + (e & 3) + 8 (e >> 2)
    uint8_t cj[2], ci[2][16];                                  // padded rows have class ROW_OUT (cls is [n_pad], zero-filled)
#pragma unroll
    for (int b = 0; b < 2; b++) cj[b] = cls[jb + 32 * b];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int e = 0; e < 16; e++) ci[a][e] = cls[ib + 32 * a + (e & 3) + 8 * (e >> 2)];
#define SIM_PASS(a, b, e) ({ const int64_t i_ = ib + 32 * (a) + ((e) & 3) + 8 * ((e) >> 2), j_ = jb + 32 * (b); \
        i_ < j_ && i_ < r1 && j_ < n && ci[a][e] != ROW_OUT && cj[b] != ROW_OUT && (((ci[a][e] | cj[b]) & ROW_WILD) || (double)acc[a][b][e] > cut); })
    __shared__ u64 room[5];                                    // [w]: candidates of wave w, then where it writes; [4]: the block's base
    u64 mine = 0;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) mine += (u64)__popcll(ballot(SIM_PASS(a, b, e)));
    if (lane == 0) room[w] = mine;
    __syncthreads();
    if (t == 0) {
        const u64 total = room[0] + room[1] + room[2] + room[3];
        room[4] = total ? atomicAdd(counter, total) : 0;
    }
    __syncthreads();
    u64 at = room[4];
    for (int q = 0; q < w; q++) at += room[q];
    const u64 below = lanes_below(lane);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const bool pass = SIM_PASS(a, b, e);
                const u64 m = ballot(pass);
                const u64 slot = at + (u64)__popcll(m & below);
                if (pass && slot < cap) cand[slot] = ((u64)(ib + 32 * a + (e & 3) + 8 * (e >> 2)) << 32) | (u64)(jb + 32 * b);
                at += (u64)__popcll(m);
            }
#undef SIM_PASS
}

// ---------------------------------------------------------------------------------------------------------------
// One thread per candidate: the reference's chain, then the strict test.  Survivors are appended (unordered).
__global__ __launch_bounds__(256) void sim_exact_kernel(const double* __restrict__ x, const double* __restrict__ norm, int dim, int metric, double threshold,
                                                        const u64* __restrict__ cand, u64 ncand, u64* __restrict__ out_key, double* __restrict__ out_sim, u64* counter)
{
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool pass = false;
    u64 key = 0;
    double sim = 0.0;
    if (c < ncand) {
        key = cand[c];
        const int64_t i = (int64_t)(key >> 32), j = (int64_t)(key & 0xffffffffull);
        sim = screen_exact_dot(x + i * dim, x + j * dim, dim) / (norm[i] * norm[j]);   // NormalizedDotProductMetric.distance: dot / (twoNorm * twoNorm)
        if (metric == MVHDP_SIM_COS_FOLDED) sim = 1.0 - fabs(1.0 - sim);   // FLOW:1483
        pass = sim > threshold;                                // NaN compares false, as in Java
    }
    const u64 slot = wave_append_slot(pass, counter, lane);
    if (pass) { out_key[slot] = key; out_sim[slot] = sim; }    // the buffers hold ncand entries
}

// ---------------------------------------------------------------------------------------------------------------
// Maths.jensenShannonDivergence, one thread per pair of a 16 x 16 tile, the rows through LDS in slabs of 32 topics.
__global__ __launch_bounds__(256) void sim_jsd_kernel(const double* __restrict__ x, const uint8_t* __restrict__ cls, int n, int dim, int r0, int r1, double threshold,
                                                      u64* __restrict__ out_key, double* __restrict__ out_sim, u64 cap, u64* counter)
{
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (tb < ta) return;
    __shared__ double P[SIM_JSD_TILE][SIM_JSD_BK + 1], Q[SIM_JSD_TILE][SIM_JSD_BK + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63;
    const int64_t i0 = (int64_t)r0 + ta * SIM_JSD_TILE, j0 = (int64_t)r0 + tb * SIM_JSD_TILE;
    const int64_t i = i0 + ty, j = j0 + tx;
    double klp = 0.0, klq = 0.0;
    bool infp = false, infq = false;
    for (int k0 = 0; k0 < dim; k0 += SIM_JSD_BK) {
        __syncthreads();
        for (int idx = t; idx < SIM_JSD_TILE * SIM_JSD_BK; idx += 256) {
            const int row = idx >> 5, kk = idx & 31;
            const bool in = k0 + kk < dim;
            P[row][kk] = (in && i0 + row < n) ? x[(i0 + row) * dim + k0 + kk] : 0.0;
            Q[row][kk] = (in && j0 + row < n) ? x[(j0 + row) * dim + k0 + kk] : 0.0;
        }
        __syncthreads();
        const int kn = dim - k0 < SIM_JSD_BK ? dim - k0 : SIM_JSD_BK;
        for (int kk = 0; kk < kn; kk++) {
            const double p = P[ty][kk], q = Q[tx][kk];
            if (p == 0.0 && q == 0.0) continue;                // neither klDivergence loop has a term here
            const double m = 0.0 + (p + q) / 2.0;              // average[i] += (p1[i] + p2[i]) / 2 on a fresh array
            if (p != 0.0) { if (m == 0.0) infp = true; else klp = klp + p * log(p / m); }   // klDivergence: skip p == 0; +inf when m == 0
            if (q != 0.0) { if (m == 0.0) infq = true; else klq = klq + q * log(q / m); }
        }
    }
    const double ln2 = 0.6931471805599453;                     // Maths.log2 = Math.log(2)
    const double a = infp ? INFINITY : klp / ln2, b = infq ? INFINITY : klq / ln2;
    const double sim = (a + b) / 2.0;
    const bool pass = i < j && i < r1 && j < n && cls[i] != ROW_OUT && cls[j] != ROW_OUT && sim > threshold;
    const u64 slot = wave_append_slot(pass, counter, lane);
    if (pass && slot < cap) { out_key[slot] = ((u64)i << 32) | (u64)j; out_sim[slot] = sim; }
}

// ---------------------------------------------------------------------------------------------------------------
// The thresholded lists.  prop: [nd][K] proportions of a chunk of entities; one wave per entity, the row in LDS.
// kept(k) <=> prop[k] >= threshold and rank(k) < maxn, rank(k) = the number of k' with prop[k'] >= threshold that IDSorter.compareTo puts
// before k: a larger weight, or the same weight and a LARGER topic id.
__device__ __forceinline__ int top_rank(const double* row, int K, int k, double threshold)
{
    const double w = row[k];
    int rank = 0;
    for (int q = 0; q < K; q++) {
        const double v = row[q];
        rank += (v >= threshold && (v > w || (v == w && q > k))) ? 1 : 0;
    }
    return rank;
}

__global__ __launch_bounds__(64) void top_count_kernel(const double* __restrict__ prop, int64_t nd, int K, double threshold, int maxn, int32_t* __restrict__ cnt)
{
    const int lane = threadIdx.x;
    for (int64_t d = blockIdx.x; d < nd; d += gridDim.x) {
        const double* row = prop + d * K;
        int c = 0;
        for (int k = lane; k < K; k += WV) c += row[k] >= threshold ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) cnt[d] = c < maxn ? c : maxn;
    }
}

// by_topic = 0: entries in list order (rank), weights as they are.  by_topic = 1: the kept entries in ascending topic id, weights rounded
// as the flow stores them, floor(w * 10^4 + 0.5) / 10^4 (PTM:2919).
__global__ __launch_bounds__(64) void top_fill_kernel(const double* __restrict__ prop, int64_t nd, int K, double threshold, int maxn, int by_topic,
                                                      const int64_t* __restrict__ off /* of this chunk's entities, absolute */, int32_t* __restrict__ topics, double* __restrict__ weights)
{
    extern __shared__ double top_lds[];
    double* row = top_lds;                                     // [K]
    uint8_t* kept = (uint8_t*)(top_lds + K);                   // [K]
    const int lane = threadIdx.x;
    for (int64_t d = blockIdx.x; d < nd; d += gridDim.x) {
        __syncthreads();
        for (int k = lane; k < K; k += WV) row[k] = prop[d * K + k];
        __syncthreads();
        const int64_t base = off[d];
        for (int k = lane; k < K; k += WV) {
            const double w = row[k];
            int rank = -1;
            if (w >= threshold) rank = top_rank(row, K, k, threshold);
            const bool keep = rank >= 0 && rank < maxn;
            kept[k] = keep ? 1 : 0;
            if (keep && !by_topic) { topics[base + rank] = k; weights[base + rank] = w; }
        }
        if (by_topic) {
            __syncthreads();
            for (int k = lane; k < K; k += WV) {
                if (!kept[k]) continue;
                int pos = 0;
                for (int q = 0; q < k; q++) pos += kept[q];
                topics[base + pos] = k;
                weights[base + pos] = floor(row[k] * 10000.0 + 0.5) / 10000.0;
            }
        }
    }
}

// One wave per group.  sum[k]: per topic the chain over the members in order (a member holds a topic at most once, so the lanes of one
// member never meet); total: ONE chain over the members in order and, within a member, ascending topic -- every lane walks it through
// the wave's registers, so every lane holds the same bits.
__global__ __launch_bounds__(64) void group_sum_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ topics, const double* __restrict__ weights,
                                                       int64_t n_groups, const int64_t* __restrict__ member_off, const int64_t* __restrict__ members,
                                                       int K, double scale /* 10^digits, or 0: no rounding */, double* __restrict__ out)
{
    extern __shared__ double sum[];                            // [K]
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        __syncthreads();
        for (int k = lane; k < K; k += WV) sum[k] = 0.0;
        __syncthreads();
        double total = 0.0;
        for (int64_t mi = member_off[g]; mi < member_off[g + 1]; mi++) {
            const int64_t d = members[mi], b = off[d], e = off[d + 1];
            for (int64_t base = b; base < e; base += WV) {
                const bool have = base + lane < e;
                const double w = have ? weights[base + lane] : 0.0;
                if (have) { const int tk = topics[base + lane]; sum[tk] = sum[tk] + w; }
                const int cnt = e - base < WV ? (int)(e - base) : WV;
                for (int l = 0; l < cnt; l++) total = total + __shfl(w, l);
            }
            __syncthreads();
        }
        for (int k = lane; k < K; k += WV) {
            double v = 0.0;
            if (total != 0.0) {
                v = sum[k] / total;
                if (scale != 0.0) v = floor(v * scale + 0.5) / scale;
            }
            out[g * K + k] = v;
        }
    }
}

struct KeySim { u64 key; double sim; };

// The lists of entities [d0, d1) as CSR arrays on the device.  Two passes over chunks of entities (counts, then entries) so that the
// dense [D][K] matrix never exists; a range that fits one chunk keeps its proportions between the passes.
struct TopCsr { DevArray<int64_t> off; DevArray<int32_t> topics; DevArray<double> weights; std::vector<int64_t> h_off; int64_t total = 0; bool over_cap = false; };

int build_top_csr(mvhdp_ctx* h, const double* view_weights, int64_t d0, int64_t d1, double threshold, int maxn, int by_topic, int64_t cap /* < 0: none */, TopCsr& csr)
{
    MvModel& mm = h->mm;
    const int K = mm.K;
    const int64_t nd = d1 - d0;
    DocTopicCarry carry{};
    int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
    csr.h_off.assign((size_t)nd + 1, 0);
    csr.total = 0;
    if (nd == 0) return MVHDP_OK;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nd, ((int64_t)256 << 20) / ((int64_t)K * 8)));
    DevArray<double> w, prop;
    DevArray<int32_t> cnt;
    HIPC(h, w.alloc((size_t)mm.M));
    HIPC(h, prop.alloc((size_t)chunk * K));
    HIPC(h, cnt.alloc((size_t)nd));
    HIPC(h, w.upload(view_weights, (size_t)mm.M, h->stream));
    auto grid = [](int64_t n) { return dim3((unsigned)(n < 16384 ? n : 16384)); };
    for (int64_t c0 = d0; c0 < d1; c0 += chunk) {
        const int64_t c1 = std::min(c0 + chunk, d1);
        HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, w, c0, c1, prop, h->stream));
        LAUNCH(h, top_count_kernel, grid(c1 - c0), dim3(WV), 0, h->stream, prop, c1 - c0, K, threshold, maxn, cnt + (c0 - d0));
    }
    std::vector<int32_t> h_cnt((size_t)nd);
    HIPC(h, cnt.download(h_cnt.data(), (size_t)nd, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (int64_t d = 0; d < nd; d++) csr.h_off[(size_t)d + 1] = csr.h_off[(size_t)d] + h_cnt[(size_t)d];
    csr.total = csr.h_off[(size_t)nd];
    if (cap >= 0 && csr.total > cap) { csr.over_cap = true; return MVHDP_OK; }
    HIPC(h, csr.off.alloc((size_t)nd + 1));
    HIPC(h, csr.topics.alloc((size_t)csr.total));
    HIPC(h, csr.weights.alloc((size_t)csr.total));
    HIPC(h, csr.off.upload(csr.h_off.data(), (size_t)nd + 1, h->stream));
    const size_t lds = (size_t)K * sizeof(double) + (size_t)K;
    for (int64_t c0 = d0; c0 < d1; c0 += chunk) {
        const int64_t c1 = std::min(c0 + chunk, d1);
        if (chunk < nd) HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, w, c0, c1, prop, h->stream));
        LAUNCH(h, top_fill_kernel, grid(c1 - c0), dim3(WV), lds, h->stream, prop, c1 - c0, K, threshold, maxn, by_topic, csr.off + (c0 - d0), csr.topics, csr.weights);
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

int top_max(int32_t max, int K) { return (max < 0 || max > K) ? K : max; }   // PTM:2867-2869

} // namespace

// ---------------------------------------------------------------------------------------------------------------
int mvhdp_screen_prepare_rows(mvhdp_ctx* h, ScreenRows& r, int64_t n, int dim, double min_weight, int64_t pad_rows, bool image)
{
    const int64_t ld = screen_ld(dim);
    HIPC(h, r.norm.alloc((size_t)n));
    HIPC(h, r.cls.alloc((size_t)(n + pad_rows)));
    if (image) HIPC(h, r.xn.alloc((size_t)(n + pad_rows) * ld));
    HIPC(h, r.cls.fill(0, h->stream));
    if (image) HIPC(h, r.xn.fill(0, h->stream));
    if (n == 0) return MVHDP_OK;
    LAUNCH(h, sim_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, r.x, (int)n, dim, min_weight, r.norm, r.cls);
    if (!image) return MVHDP_OK;
    const int64_t cells = n * dim;
    LAUNCH(h, sim_normalise_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->stream, r.x, r.norm, r.cls, (int)n, dim, ld, r.xn);
    return MVHDP_OK;
}

extern "C" int mvhdp_sim_probe(int32_t n, int32_t dim, int32_t stripe_rows, mvhdp_sim_stats* out)
{
    if (!out || n < 0 || dim < 1 || stripe_rows < 0) return MVHDP_ERR_INVALID_ARG;
    if (dim > SIM_MAX_DIM) return MVHDP_ERR_UNSUPPORTED;
    memset(out, 0, sizeof *out);
    out->margin = sim_margin(dim);
    out->stripes = sim_stripes(n, stripe_rows);
    out->pairs_screened = sim_cells(n, stripe_rows, SCREEN_TILE);
    return MVHDP_OK;
}

extern "C" int mvhdp_similar_pairs(mvhdp_handle h, const mvhdp_sim_args* a, int64_t cap, int32_t* oi, int32_t* oj, double* osim, int64_t* count, mvhdp_sim_stats* stats)
{
    CHECK_H(h);
    if (!a || !count || cap < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: null argument or negative cap");
    if (a->metric < MVHDP_SIM_COS_FOLDED || a->metric > MVHDP_SIM_JSD) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: unknown metric");
    if (a->n < 0 || a->dim < 1 || (a->n > 0 && !a->x)) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: bad shape or null x");
    if (!(a->threshold >= 0.0) || !(a->threshold < INFINITY)) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: threshold must be finite and >= 0");
    if (a->min_weight != a->min_weight) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: min_weight is NaN");
    if (a->stripe_rows < 0 || a->candidate_capacity < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: negative stripe_rows or candidate_capacity");
    if (cap > 0 && (!oi || !oj || !osim)) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: cap > 0 with a null output");
    if (a->dim > SIM_MAX_DIM) FAIL(h, MVHDP_ERR_UNSUPPORTED, "similar_pairs: dim > 65536 (the screen's margin would reach 0.01)");
    const bool jsd = a->metric == MVHDP_SIM_JSD;
    const int n = a->n, dim = a->dim, tile = jsd ? SIM_JSD_TILE : SCREEN_TILE;
    const int64_t S = sim_stripe_rows(a->stripe_rows);
    mvhdp_sim_stats st{};
    st.margin = jsd ? 0.0 : sim_margin(dim);
    st.stripes = sim_stripes(n, a->stripe_rows);
    st.pairs_screened = sim_cells(n, a->stripe_rows, tile);
    *count = 0;
    if (n < 2) { if (stats) *stats = st; return MVHDP_OK; }
    HIPC(h, hipSetDevice(h->device));

    // rows are padded so that every tile of every stripe reads inside the image: a stripe may start at any row.  JSD has no image.
    const int64_t ld = screen_ld(dim);
    ScreenRows R;
    DevArray<double> ssim;
    DevArray<u64> ctr, cand, skey;
    HIPC(h, R.x.alloc((size_t)n * dim));
    HIPC(h, ctr.alloc(2));
    HIPC(h, R.x.upload(a->x, (size_t)n * dim, h->stream));
    int rc = mvhdp_screen_prepare_rows(h, R, n, dim, a->min_weight, 2 * SCREEN_TILE, !jsd); if (rc) return rc;
    u64 ccap = (u64)(a->candidate_capacity > 0 ? a->candidate_capacity : SIM_AUTO_CAPACITY);
    auto size_buffers = [&](u64 c) -> hipError_t {
        hipError_t e = skey.alloc((size_t)c);
        if (e == hipSuccess) e = ssim.alloc((size_t)c);
        if (e == hipSuccess && !jsd) e = cand.alloc((size_t)c);
        return e;
    };
    HIPC(h, size_buffers(ccap));
    const double cut = a->threshold - st.margin;
    std::vector<KeySim> stripe;
    std::vector<u64> hk;
    std::vector<double> hs;
    int64_t emitted = 0;
    bool over = false;
    for (int64_t r0 = 0; r0 < n; r0 += S) {
        const int64_t r1 = std::min<int64_t>(r0 + S, n);
        int64_t na, nb;
        sim_stripe_tiles(n, r0, r1, tile, &na, &nb);
        const dim3 grid((unsigned)nb, (unsigned)na);
        u64 hc[2] = {0, 0};
        for (int attempt = 0; ; attempt++) {
            HIPC(h, ctr.fill(0, h->stream));
            if (jsd)
                LAUNCH(h, sim_jsd_kernel, grid, dim3(256), 0, h->stream, R.x, R.cls, n, dim, (int)r0, (int)r1, a->threshold, skey, ssim, ccap, ctr);
            else
                LAUNCH(h, sim_screen_kernel, grid, dim3(256), 0, h->stream, R.xn, ld, (int)(ld / SCREEN_BK), R.cls, n, (int)r0, (int)r1, cut, cand, ccap, ctr);
            HIPC(h, ctr.download(hc, 2, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
            if (hc[0] <= ccap) break;
            if (attempt) FAIL(h, MVHDP_ERR_HIP, "similar_pairs: a stripe asked for more room twice");   // the count is a function of the data alone
            ccap = hc[0];                                      // redo the stripe with the room it asked for
            st.regrown++;
            HIPC(h, size_buffers(ccap));
        }
        u64 nsurv = hc[0];
        if (!jsd) {
            st.candidates += (int64_t)hc[0];
            if (hc[0]) {
                LAUNCH(h, sim_exact_kernel, dim3((unsigned)((hc[0] + 255) / 256)), dim3(256), 0, h->stream, R.x, R.norm, dim, a->metric, a->threshold,
                       cand, hc[0], skey, ssim, ctr + 1);
                HIPC(h, ctr.download(hc, 2, h->stream));
                HIPC(h, hipStreamSynchronize(h->stream));
            }
            nsurv = hc[1];
        } else
            st.candidates += (int64_t)nsurv;
        if (nsurv && !over && emitted + (int64_t)nsurv <= cap) {
            hk.resize((size_t)nsurv); hs.resize((size_t)nsurv);
            HIPC(h, skey.download(hk.data(), (size_t)nsurv, h->stream));
            HIPC(h, ssim.download(hs.data(), (size_t)nsurv, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
            const size_t at = stripe.size();
            stripe.resize(at + (size_t)nsurv);
            for (size_t q = 0; q < (size_t)nsurv; q++) stripe[at + q] = KeySim{hk[q], hs[q]};
            std::sort(stripe.begin() + at, stripe.end(), [](const KeySim& l, const KeySim& r) { return l.key < r.key; });   // stripes come in row order
        } else if (emitted + (int64_t)nsurv > cap)
            over = true;
        emitted += (int64_t)nsurv;
    }
    st.emitted = emitted;
    *count = emitted;
    if (stats) *stats = st;
    if (over && !(cap == 0 && !oi && !oj && !osim)) FAIL(h, MVHDP_ERR_INVALID_ARG, "similar_pairs: more pairs than cap (count is set)");
    if (over) return MVHDP_OK;                                 // the count-only call
    for (size_t q = 0; q < stripe.size(); q++) {
        oi[q] = (int32_t)(stripe[q].key >> 32); oj[q] = (int32_t)(stripe[q].key & 0xffffffffull); osim[q] = stripe[q].sim;
    }
    return MVHDP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" int mvhdp_doc_topics_top(mvhdp_handle h, const double* view_weights, int64_t d0, int64_t d1, double threshold, int32_t max,
                                    int64_t cap, int64_t* row_off, int32_t* topics, double* weights, int64_t* count)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (!view_weights || !count || cap < 0 || d0 < 0 || d1 > mm.D || d0 > d1) FAIL(h, MVHDP_ERR_INVALID_ARG, "doc_topics_top: bad range, null buffer or negative cap");
    if (threshold != threshold) FAIL(h, MVHDP_ERR_INVALID_ARG, "doc_topics_top: threshold is NaN");
    if (cap > 0 && (!topics || !weights)) FAIL(h, MVHDP_ERR_INVALID_ARG, "doc_topics_top: cap > 0 with a null output");
    const bool count_only = cap == 0 && !topics && !weights;
    TopCsr csr;
    int rc = build_top_csr(h, view_weights, d0, d1, threshold, top_max(max, mm.K), 0, count_only ? -1 : cap, csr);
    if (rc) return rc;
    *count = csr.total;
    if (csr.over_cap) FAIL(h, MVHDP_ERR_INVALID_ARG, "doc_topics_top: more entries than cap (count is set)");
    if (!count_only && csr.total > 0) {
        HIPC(h, csr.topics.download(topics, (size_t)csr.total, h->stream));
        HIPC(h, csr.weights.download(weights, (size_t)csr.total, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    if (row_off) memcpy(row_off, csr.h_off.data(), csr.h_off.size() * sizeof(int64_t));
    return MVHDP_OK;
}

extern "C" int mvhdp_entity_topic_distributions(mvhdp_handle h, const double* view_weights, double threshold, int32_t max, int32_t round_digits,
                                                int64_t n_groups, const int64_t* member_off, const int64_t* members, double* out)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (!view_weights || n_groups < 0 || !member_off || (n_groups > 0 && !out)) FAIL(h, MVHDP_ERR_INVALID_ARG, "entity_topic_distributions: null buffer or negative n_groups");
    if (threshold != threshold || round_digits < -1 || round_digits > 15) FAIL(h, MVHDP_ERR_INVALID_ARG, "entity_topic_distributions: NaN threshold or round_digits outside -1..15");
    if (const char* r = check_offsets(member_off, n_groups, INT64_MAX)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("entity_topic_distributions: member_off ") + r);
    const int64_t nm = member_off[n_groups];
    if (nm > 0 && !members) FAIL(h, MVHDP_ERR_INVALID_ARG, "entity_topic_distributions: null members");
    for (int64_t q = 0; q < nm; q++)
        if (members[q] < 0 || members[q] >= mm.D) FAIL(h, MVHDP_ERR_INVALID_ARG, "entity_topic_distributions: member outside [0, D)");
    TopCsr csr;
    int rc = build_top_csr(h, view_weights, 0, mm.D, threshold, top_max(max, K), 1, -1, csr);
    if (rc) return rc;
    if (n_groups == 0) return MVHDP_OK;
    if (mm.D == 0) {                                           // no entity, so no member: rows of zeros
        for (int64_t q = 0; q < n_groups * K; q++) out[q] = 0.0;
        return MVHDP_OK;
    }
    double scale = 0.0;
    if (round_digits >= 0) { scale = 1.0; for (int q = 0; q < round_digits; q++) scale = scale * 10.0; }   // exact: 10^15 < 2^53
    DevArray<int64_t> moff, mem;
    DevArray<double> dout;
    HIPC(h, moff.alloc((size_t)n_groups + 1));
    HIPC(h, mem.alloc((size_t)nm));
    HIPC(h, dout.alloc((size_t)n_groups * K));
    HIPC(h, moff.upload(member_off, (size_t)n_groups + 1, h->stream));
    if (nm) HIPC(h, mem.upload(members, (size_t)nm, h->stream));
    LAUNCH(h, group_sum_kernel, dim3((unsigned)(n_groups < 16384 ? n_groups : 16384)), dim3(WV), (size_t)K * sizeof(double), h->stream,
           csr.off, csr.topics, csr.weights, n_groups, moff, mem, K, scale, dout);
    HIPC(h, dout.download(out, (size_t)n_groups * K, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}
