// mvhdp_gram.hip — the topic map: K x K sums over a tall matrix with K columns, X = theta of the handle's entities, phi of one view, or the
// caller's rows (include/mvhdp.h has the contract: the blocks of 1024 rows, the chains, the order of the blocks, the counts;
// tests/native/gram_ref.c restates it on the host).  y = X or sqrt(X).
//   gram_sqrt_kernel      y = sqrt(x) in place over the staged rows, correctly rounded; behind the counts, which are taken on X.
//   gram_block_kernel     the hot one.  A workgroup of 256 threads owns one block of rows and one tile of 64 (k) x 128 (l) cells; thread
//                         (ty, tx) holds 4 x 8 fp64 accumulators, the layout and the inner loop of xview_score_kernel (slab_fma of
//                         mvhdp_xview.h).  Rows stream through LDS in slabs of 16.  X is row-major over the topics, so a slab
//                         [16 rows][topics] is already the [chain index][cell] layout that kernel transposes into: the staging is a plain
//                         copy, 64 (128) consecutive doubles of a row per 64 (128) threads, and both operands are columns of the same rows.
//                         The next slab is in flight in registers while this one is multiplied.  Every accumulator is ONE chain
//                         p = fma(y_r[k], y_r[l], p) from +0.0 over the block's rows ascending: no partial sums inside a block.  Only tiles
//                         that hold a cell with k <= l are launched; the partial of block b goes to P[b][k][l].
//   gram_colsum_kernel    q = q + y_r[k] over a block's rows ascending: one thread per (block, topic), lanes over topics.
//   gram_reduce_kernel    after each pass: gram[k][l] = gram[k][l] + P[b][k][l] for the pass's blocks ascending, one thread per cell with
//                         k <= l (the host mirrors the finished table); sums[k] likewise.  The device tables carry over the passes.
//   gram_mask_kernel      a workgroup per block of rows and 64 topics: 64 rows x 64 topics of (X > threshold) through LDS, then per topic
//                         a ballot over the 64 rows gives the 64-bit mask of rows above; 16 such words per topic and block.  Their
//                         popcounts add into n_above.
//   gram_co_kernel        co_above[k][l] grows by popcount(mask_k & mask_l): a workgroup per 64 x 64 tile with a cell k <= l and per share
//                         of the pass's 64-row groups, a thread 4 x 4 cells; the cost does not depend on how many rows lie above.
// The integer tables grow by 64-bit integer atomics, which commute; there are no floating-point atomics.  Everything runs on the handle's
// stream; theta (mvhdp_launch_doc_topic_prop) and phi (xview_phi_kernel) are formed per pass and never leave the device.
#include "mvhdp_side.h"
#include "mvhdp_select.h"
#include "mvhdp_xview.h"

namespace {

constexpr int GRAM_B = MVHDP_GRAM_BLOCK_ROWS;
constexpr int GRAM_GROUPS = GRAM_B / 64;                       // 64-row mask words per topic and block
constexpr int64_t GRAM_PARTIAL_BYTES = (int64_t)256 << 20;     // the block partials of a pass
constexpr int64_t GRAM_ROWS_BYTES = (int64_t)1 << 30;          // the rows of a pass
constexpr int64_t GRAM_MAX_PASS_BLOCKS = (int64_t)1 << 20;     // grid = blocks x tiles stays below 2^31 up to MVHDP_MAX_TOPICS
constexpr int CO_T = 64, CO_GS = 16;                           // co-occurrence tile edge; groups staged at once
static_assert(GRAM_B % XV_KS == 0 && GRAM_B % 64 == 0, "a block is whole slabs and whole mask words");

__global__ __launch_bounds__(256) void gram_sqrt_kernel(double* __restrict__ y, int64_t cells)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) y[i] = __builtin_sqrt(y[i]);
}

struct GramArgs {
    const double* y;                   // [rows][K] of the pass
    double* P;                         // [blocks][K][K]
    const int32_t* tiles;              // [ntiles][2]: tile row (64 cells of k), tile column (128 cells of l)
    int64_t rows;
    int32_t K, ntiles;
};

__global__ __launch_bounds__(256) void gram_block_kernel(const GramArgs a)
{
    __shared__ __attribute__((aligned(16))) double th[XV_KS][XV_BE + 2];
    __shared__ __attribute__((aligned(16))) double ph[XV_KS][XV_BW + 2];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)a.ntiles);
    const int tile = (int)(blockIdx.x % (unsigned)a.ntiles);
    const int k0 = a.tiles[2 * tile] * XV_BE, l0 = a.tiles[2 * tile + 1] * XV_BW;
    const int K = a.K;
    const int64_t rb = b * GRAM_B;
    const int nr = (int)(a.rows - rb < GRAM_B ? a.rows - rb : GRAM_B);
    const double* __restrict__ y = a.y + rb * K;
    // staging: thread t moves topic k0 + (t & 63) of slab rows (t >> 6) + 4 i, and topic l0 + (t & 127) of slab rows (t >> 7) + 2 i
    const int ck = t & (XV_BE - 1), rk = t >> 6, cl = t & (XV_BW - 1), rl = t >> 7;
    const bool okk = k0 + ck < K, okl = l0 + cl < K;
    double rt[XV_KS / 4], rp[XV_KS / 2];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int i = 0; i < XV_KS / 4; i++) { const int r = r0 + rk + 4 * i; rt[i] = (okk && r < nr) ? y[(int64_t)r * K + k0 + ck] : 0.0; }
#pragma unroll
        for (int i = 0; i < XV_KS / 2; i++) { const int r = r0 + rl + 2 * i; rp[i] = (okl && r < nr) ? y[(int64_t)r * K + l0 + cl] : 0.0; }
    };
    double acc[XV_TE][XV_TW];
#pragma unroll
    for (int i = 0; i < XV_TE; i++)
#pragma unroll
        for (int j = 0; j < XV_TW; j++) acc[i][j] = 0.0;

    fetch(0);
    for (int r0 = 0; r0 < nr; r0 += XV_KS) {                   // ascending rows: the order of the chain
#pragma unroll
        for (int i = 0; i < XV_KS / 4; i++) th[rk + 4 * i][ck] = rt[i];
#pragma unroll
        for (int i = 0; i < XV_KS / 2; i++) ph[rl + 2 * i][cl] = rp[i];
        __syncthreads();
        if (r0 + XV_KS < nr) fetch(r0 + XV_KS);
        const int kn = nr - r0;
        if (kn >= XV_KS) slab_fma<true>(th, ph, XV_KS, ty, tx, acc);
        else slab_fma<false>(th, ph, kn, ty, tx, acc);          // the rows beyond the block are never multiplied
        __syncthreads();
    }
    double* __restrict__ P = a.P + b * K * K;
#pragma unroll
    for (int i = 0; i < XV_TE; i++) {
        const int k = k0 + ty * XV_TE + i;
        if (k >= K) continue;
#pragma unroll
        for (int j = 0; j < XV_TW; j++) {
            const int l = l0 + 2 * tx + 16 * (j & ~1) + (j & 1);
            if (l < K) P[(int64_t)k * K + l] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void gram_colsum_kernel(const double* __restrict__ y, int64_t rows, int K, int64_t nb, double* __restrict__ Psum)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb * K) return;
    const int64_t b = i / K, rb = b * GRAM_B;
    const int k = (int)(i - b * K);
    const int nr = (int)(rows - rb < GRAM_B ? rows - rb : GRAM_B);
    const double* __restrict__ p = y + rb * K + k;
    double q = 0.0;
#pragma unroll 8
    for (int r = 0; r < nr; r++) q = q + p[(int64_t)r * K];
    Psum[i] = q;
}

__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ P, const double* __restrict__ Psum, int64_t nb, int K, double* __restrict__ gram,
                                                          double* __restrict__ sums)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, KK = (int64_t)K * K;
    if (i < KK) {
        if (i / K > i % K) return;                             // below the diagonal: the host mirrors
        double g = gram[i];
        for (int64_t b = 0; b < nb; b++) g = g + P[b * KK + i];
        gram[i] = g;
    } else if (i < KK + K) {
        const int64_t k = i - KK;
        double q = sums[k];
        for (int64_t b = 0; b < nb; b++) q = q + Psum[b * K + k];
        sums[k] = q;
    }
}

// masks[(16 b + g)][k]: bit r of the word = X[64 (16 b + g) + r][k] > threshold, rows of the pass
__global__ __launch_bounds__(256) void gram_mask_kernel(const double* __restrict__ x, int64_t rows, int K, int ktiles, double threshold, u64* __restrict__ masks,
                                                        u64* __restrict__ n_above)
{
    __shared__ uint32_t above[64][65];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)ktiles);
    const int k0 = (int)(blockIdx.x % (unsigned)ktiles) * 64;
    const int64_t rb = b * GRAM_B;
    const int nr = (int)(rows - rb < GRAM_B ? rows - rb : GRAM_B);
    const bool okc = k0 + lane < K;
    const int k = k0 + 16 * w + lane;                          // the topic lanes 0..15 of wave w answer for
    int cnt = 0;
    for (int g = 0; g * 64 < nr; g++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = g * 64 + w + 4 * i;
            above[w + 4 * i][lane] = (okc && r < nr && x[(rb + r) * K + k0 + lane] > threshold) ? 1u : 0u;
        }
        __syncthreads();
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const u64 m = ballot(above[lane][16 * w + j] != 0u);
            if (lane == j) mine = m;
        }
        if (lane < 16 && k < K) { masks[(b * GRAM_GROUPS + g) * K + k] = mine; cnt += __popcll(mine); }
        __syncthreads();
    }
    if (lane < 16 && k < K && cnt) atomicAdd(&n_above[k], (u64)cnt);
}

// a workgroup: tile `tile` of 64 x 64 cells over the groups [chunk * gper, (chunk + 1) * gper) of the pass
__global__ __launch_bounds__(256) void gram_co_kernel(const u64* __restrict__ masks, int64_t G, int K, const int32_t* __restrict__ tiles, int ntiles, int64_t gper,
                                                      u64* __restrict__ co)
{
    __shared__ u64 mk[CO_GS][CO_T], ml[CO_GS][CO_T];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int tile = (int)(blockIdx.x % (unsigned)ntiles);
    const int64_t chunk = (int64_t)(blockIdx.x / (unsigned)ntiles);
    const int k0 = tiles[2 * tile] * CO_T, l0 = tiles[2 * tile + 1] * CO_T;
    const int64_t gb = chunk * gper, ge = gb + gper < G ? gb + gper : G;
    const int sc = t & 63, sr = t >> 6;
    uint32_t c[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[i][j] = 0u;
    for (int64_t g0 = gb; g0 < ge; g0 += CO_GS) {
#pragma unroll
        for (int i = 0; i < CO_GS / 4; i++) {
            const int64_t g = g0 + sr + 4 * i;
            mk[sr + 4 * i][sc] = (g < ge && k0 + sc < K) ? masks[g * K + k0 + sc] : 0ull;
            ml[sr + 4 * i][sc] = (g < ge && l0 + sc < K) ? masks[g * K + l0 + sc] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < CO_GS; q++) {
            u64 a[4], bb[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = mk[q][4 * ty + i]; bb[i] = ml[q][4 * tx + i]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) c[i][j] += (uint32_t)__popcll(a[i] & bb[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k0 + 4 * ty + i, l = l0 + 4 * tx + j;
            if (k <= l && l < K && c[i][j]) atomicAdd(&co[(int64_t)k * K + l], (u64)c[i][j]);
        }
}

// every check comes before the first output is touched
int check_args(mvhdp_ctx* h, const mvhdp_topic_gram_args* a, const double* gram, const double* sums)
{
    MvModel& mm = h->mm;
    if (!a || !gram || !sums) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: null arguments, gram or sums");
    if (a->source != MVHDP_GRAM_ENTITIES && a->source != MVHDP_GRAM_WORDS && a->source != MVHDP_GRAM_HOST) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad source");
    if (a->transform != MVHDP_GRAM_IDENTITY && a->transform != MVHDP_GRAM_SQRT) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad transform");
    if (a->blocks_per_pass < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: negative blocks_per_pass");
    if (std::isnan(a->threshold)) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: NaN threshold");
    if (a->source == MVHDP_GRAM_HOST) {
        if (!a->x) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: null x");
        if (a->r0 < 0 || a->r0 > a->r1) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad row range");
        if (const char* r = check_nonneg_finite(a->x, (a->r1 - a->r0) * mm.K)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("topic_gram: an x entry ") + r);
        return MVHDP_OK;
    }
    if (a->source == MVHDP_GRAM_WORDS && (a->m < 0 || a->m >= mm.M)) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad view");
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "topic_gram before set_hyper");
    if (a->source == MVHDP_GRAM_WORDS) {
        rc = require_current_counts(h, "topic_gram"); if (rc) return rc;
        if (a->r0 < 0 || a->r1 > mm.V[a->m] || a->r0 > a->r1) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad type range");
        return MVHDP_OK;
    }
    if (a->r0 < 0 || a->r1 > mm.D || a->r0 > a->r1) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_gram: bad entity range");
    if (const char* r = check_view_weights(a->view_weights, mm.M)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("topic_gram: ") + r);
    return MVHDP_OK;
}

struct GramOut {
    std::vector<double> gram, sums;
    std::vector<u64> n_above, co;
};

int gram_run(mvhdp_ctx* h, const mvhdp_topic_gram_args* a, bool want_n, bool want_co, GramOut& out, mvhdp_topic_gram_stats& st)
{
    MvModel& mm = h->mm;
    const int K = mm.K;
    const int64_t KK = (int64_t)K * K, R = a->r1 - a->r0, NB = (R + GRAM_B - 1) / GRAM_B;
    const bool counts = want_n || want_co;
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    // blocks per pass: what the caller asks for, else the partials within 256 MiB; either way the rows of a pass within 1 GiB
    int64_t BP = a->blocks_per_pass > 0 ? a->blocks_per_pass : std::max<int64_t>(1, GRAM_PARTIAL_BYTES / (KK * (int64_t)sizeof(double)));
    BP = std::min(BP, std::max<int64_t>(1, GRAM_ROWS_BYTES / ((int64_t)GRAM_B * K * (int64_t)sizeof(double))));
    BP = std::max<int64_t>(1, std::min(std::min(BP, GRAM_MAX_PASS_BLOCKS), NB));

    // the tiles that hold a cell with k <= l
    std::vector<int32_t> h_tiles, h_cotiles;
    for (int ti = 0; ti * XV_BE < K; ti++)
        for (int tj = 0; tj * XV_BW < K; tj++)
            if (ti * XV_BE <= std::min(tj * XV_BW + XV_BW - 1, K - 1)) { h_tiles.push_back(ti); h_tiles.push_back(tj); }
    for (int ti = 0; ti * CO_T < K; ti++)
        for (int tj = ti; tj * CO_T < K; tj++) { h_cotiles.push_back(ti); h_cotiles.push_back(tj); }
    const int ntiles = (int)(h_tiles.size() / 2), ncotiles = (int)(h_cotiles.size() / 2), ktiles = (K + 63) / 64;

    DocTopicCarry carry{};
    DevArray<double> d_w, d_y, d_P, d_Psum, d_gram, d_sums;
    DevArray<int32_t> d_tiles, d_cotiles;
    DevArray<u64> d_masks, d_n, d_co;
    if (a->source == MVHDP_GRAM_ENTITIES) {
        int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
        HIPC(h, d_w.alloc((size_t)mm.M));
        HIPC(h, d_w.upload(a->view_weights, (size_t)mm.M, s));
    }
    HIPC(h, d_y.alloc((size_t)(std::min(BP * GRAM_B, R) * K)));
    HIPC(h, d_P.alloc((size_t)(BP * KK)));
    HIPC(h, d_Psum.alloc((size_t)(BP * K)));
    HIPC(h, d_gram.alloc((size_t)KK));
    HIPC(h, d_sums.alloc((size_t)K));
    HIPC(h, d_gram.fill(0, s));
    HIPC(h, d_sums.fill(0, s));
    HIPC(h, d_tiles.alloc(h_tiles.size()));
    HIPC(h, d_tiles.upload(h_tiles.data(), h_tiles.size(), s));
    if (counts) {
        HIPC(h, d_masks.alloc((size_t)(BP * GRAM_GROUPS * K)));
        HIPC(h, d_n.alloc((size_t)K));
        HIPC(h, d_n.fill(0, s));
        if (want_co) {
            HIPC(h, d_co.alloc((size_t)KK));
            HIPC(h, d_co.fill(0, s));
            HIPC(h, d_cotiles.alloc(h_cotiles.size()));
            HIPC(h, d_cotiles.upload(h_cotiles.data(), h_cotiles.size(), s));
        }
    }
    StreamTimer timer;
    HIPC(h, timer.create());
    HIPC(h, timer.start(s));

    const unsigned wide = (unsigned)h->num_cus * 16;
    for (int64_t b0 = 0; b0 < NB; b0 += BP) {
        const int64_t nb = std::min(BP, NB - b0), p0 = a->r0 + b0 * GRAM_B, rows = std::min(nb * GRAM_B, a->r1 - p0), cells = rows * K;
        // ---- X of the pass ----
        if (a->source == MVHDP_GRAM_ENTITIES) HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, d_w, p0, p0 + rows, d_y, s));
        else if (a->source == MVHDP_GRAM_WORDS)
            LAUNCH(h, xview_phi_kernel, dim3((unsigned)std::min<int64_t>((cells + 255) / 256, wide)), dim3(256), 0, s, mm.counts + (mm.rowbase[a->m] + p0) * K,
                   mm.counts + mm.rowbase[mm.M] * K + (int64_t)a->m * K, mm.inactive, K, cells, mm.beta[a->m], mm.beta_sum[a->m], d_y.get());
        else HIPC(h, d_y.upload(a->x + b0 * GRAM_B * K, (size_t)cells, s));
        // ---- the integers, on X ----
        if (counts) {
            LAUNCH(h, gram_mask_kernel, dim3((unsigned)(nb * ktiles)), dim3(256), 0, s, d_y, rows, K, ktiles, a->threshold, d_masks, d_n);
            if (want_co) {
                const int64_t G = (rows + 63) / 64;
                const int64_t shares = std::max<int64_t>(1, std::min<int64_t>((G + CO_GS - 1) / CO_GS, ((int64_t)h->num_cus * 8 + ncotiles - 1) / ncotiles));
                const int64_t gper = (G + shares - 1) / shares;                 // at most 2^20 * 16 groups: a cell's 32-bit count cannot wrap
                LAUNCH(h, gram_co_kernel, dim3((unsigned)(((G + gper - 1) / gper) * ncotiles)), dim3(256), 0, s, d_masks, G, K, d_cotiles, ncotiles, gper, d_co);
            }
        }
        // ---- y, the block partials, the ordered sums ----
        if (a->transform == MVHDP_GRAM_SQRT) LAUNCH(h, gram_sqrt_kernel, dim3((unsigned)std::min<int64_t>((cells + 255) / 256, wide)), dim3(256), 0, s, d_y.get(), cells);
        GramArgs ga{};
        ga.y = d_y; ga.P = d_P; ga.tiles = d_tiles; ga.rows = rows; ga.K = K; ga.ntiles = ntiles;
        LAUNCH(h, gram_block_kernel, dim3((unsigned)(nb * ntiles)), dim3(256), 0, s, ga);
        LAUNCH(h, gram_colsum_kernel, dim3((unsigned)((nb * K + 255) / 256)), dim3(256), 0, s, d_y, rows, K, nb, d_Psum);
        LAUNCH(h, gram_reduce_kernel, dim3((unsigned)((KK + K + 255) / 256)), dim3(256), 0, s, d_P, d_Psum, nb, K, d_gram, d_sums);
        st.passes++;
    }
    HIPC(h, timer.stop(s));
    HIPC(h, d_gram.download(out.gram.data(), (size_t)KK, s));
    HIPC(h, d_sums.download(out.sums.data(), (size_t)K, s));
    if (counts) HIPC(h, d_n.download(out.n_above.data(), (size_t)K, s));
    if (want_co) HIPC(h, d_co.download(out.co.data(), (size_t)KK, s));
    HIPC(h, hipStreamSynchronize(s));
    for (int k = 1; k < K; k++)
        for (int l = 0; l < k; l++) {
            out.gram[(size_t)k * K + l] = out.gram[(size_t)l * K + k];
            if (want_co) out.co[(size_t)k * K + l] = out.co[(size_t)l * K + k];
        }
    HIPC(h, timer.elapsed_ms(&st.kernel_ms));
    st.rows = R;
    st.blocks = (int32_t)NB;
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_topic_gram(mvhdp_handle h, const mvhdp_topic_gram_args* a, double* gram, double* sums, int64_t* n_above, int64_t* co_above, mvhdp_topic_gram_stats* stats)
{
    CHECK_H(h);
    int rc = check_args(h, a, gram, sums); if (rc) return rc;
    const int K = h->mm.K;
    const size_t KK = (size_t)K * K;
    if (a->r1 - a->r0 > ((int64_t)1 << 40)) FAIL(h, MVHDP_ERR_UNSUPPORTED, "topic_gram: more than 2^40 rows");
    GramOut out;
    out.gram.assign(KK, 0.0); out.sums.assign((size_t)K, 0.0); out.n_above.assign((size_t)K, 0); out.co.assign(co_above ? KK : 0, 0);
    mvhdp_topic_gram_stats st{};
    if (a->r1 > a->r0) { rc = gram_run(h, a, n_above != nullptr, co_above != nullptr, out, st); if (rc) return rc; }
    memcpy(gram, out.gram.data(), KK * sizeof(double));
    memcpy(sums, out.sums.data(), (size_t)K * sizeof(double));
    if (n_above) memcpy(n_above, out.n_above.data(), (size_t)K * sizeof(int64_t));
    if (co_above) memcpy(co_above, out.co.data(), KK * sizeof(int64_t));
    if (stats) *stats = st;
    return MVHDP_OK;
}
