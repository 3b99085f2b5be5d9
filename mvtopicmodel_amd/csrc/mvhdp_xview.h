// mvhdp_xview.h — what mvhdp_xview.hip (types per entity) and mvhdp_xview_entities.hip (entities per item query) share: the phi table,
// the tiled fp64 score kernel and the marker of an excluded cell.  Both operands of the score kernel are K-contiguous row matrices, so either side of the
// product can take either slot: S[r][col0 + w] = the chain over k of theta[row r][k] * phi[w][k].
//   xview_phi_kernel      phi[w][k] = (n_wk + beta) / (n_k + betaSum), 0 for an inactive topic: one thread per cell of a stripe of types,
//                         fp64 [types][K], K-contiguous like the count rows.
//   xview_score_kernel    the hot one.  A block of 256 threads computes 64 entities x 128 types; thread (ty, tx) holds 4 x 8 fp64
//                         accumulators: entities 4 ty + i, types 2 tx + 32 j + {0, 1}.  theta and phi are staged in LDS in slabs of 16
//                         topics, transposed to [k][row] with a pitch of rows + 2 doubles (rows stay 16-byte aligned; the staging writes
//                         are 2-way at worst).  Per k a lane reads its 4 theta values (two 16-byte reads, the same address in 16 lanes
//                         of a wave: a broadcast) and 4 pairs of phi values (16-byte reads, 16 lanes on 256 consecutive bytes: every
//                         bank once) -- 16-byte reads on purpose: two 8-byte reads a stride apart are merged into one two-address
//                         read, which moves a quarter of the bytes per LDS cycle.  The next slab is in flight in registers while this one is multiplied.  The slabs are walked
//                         in ascending k and every accumulator is ONE chain s = fma(theta[k], phi[k], s) from +0.0: no partial sums.
// The kernels live in each including unit's unnamed namespace.
#pragma once
#include "mvhdp_ctx.h"
#include "mvhdp_select.h"

namespace {

// the bits written over an excluded cell of the block of scores: f64_bits_key gives 0, the key of an entry that does not count.  (The
// scores are read as their bits and ordered by f64_bits_key; the chain never yields -0.0: it starts at +0.0.)
constexpr u64 XV_EXCLUDED = ~0ull;
constexpr int XV_TE = 4, XV_TW = 8;                            // a thread's tile: entities x types
constexpr int XV_BE = 16 * XV_TE, XV_BW = 16 * XV_TW;          // a block's tile: 64 x 128
constexpr int XV_KS = 16;                                      // topics per slab

__global__ __launch_bounds__(256) void xview_phi_kernel(const int32_t* __restrict__ rows /*n_wk of the stripe's first type*/, const int32_t* __restrict__ nk,
                                                        const uint8_t* __restrict__ inactive, int K, int64_t cells, double beta, double beta_sum, double* __restrict__ phi)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        const int k = (int)(i % K);
        phi[i] = inactive[k] ? 0.0 : ((double)rows[i] + beta) / ((double)nk[k] + beta_sum);
    }
}

struct ScoreArgs {
    const double* theta;               // [..][K] rows of the theta range
    const int32_t* row_list;           // [n_rows] theta row of score row r, or nullptr: row0 + r
    int64_t row0;
    const double* phi;                 // [n_types][K] of the stripe
    double* S;                         // [n_rows][ldS]; the stripe's first type is column col0
    int64_t ldS, col0;
    int32_t n_rows, n_types, K, tiles_w;
};

template <bool FULL>
__device__ __forceinline__ void slab_fma(const double (*th)[XV_BE + 2], const double (*ph)[XV_BW + 2], int kn, int ty, int tx, double (&acc)[XV_TE][XV_TW])
{
#pragma unroll
    for (int kk = 0; kk < XV_KS; kk++) {
        if (!FULL && kk >= kn) break;
        double a[XV_TE], b[XV_TW];
#pragma unroll
        for (int i = 0; i < XV_TE; i += 2) {
            const double2 v = *reinterpret_cast<const double2*>(&th[kk][ty * XV_TE + i]);
            a[i] = v.x; a[i + 1] = v.y;
        }
#pragma unroll
        for (int j = 0; j < XV_TW; j += 2) {
            const double2 v = *reinterpret_cast<const double2*>(&ph[kk][2 * tx + 16 * j]);
            b[j] = v.x; b[j + 1] = v.y;
        }
#pragma unroll
        for (int i = 0; i < XV_TE; i++)
#pragma unroll
            for (int j = 0; j < XV_TW; j++) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
    }
}

__global__ __launch_bounds__(256) void xview_score_kernel(const ScoreArgs a)
{
    __shared__ __attribute__((aligned(16))) double th[XV_KS][XV_BE + 2];
    __shared__ __attribute__((aligned(16))) double ph[XV_KS][XV_BW + 2];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int e0 = (int)(blockIdx.x / (unsigned)a.tiles_w) * XV_BE, w0 = (int)(blockIdx.x % (unsigned)a.tiles_w) * XV_BW;
    const int K = a.K;
    // staging: thread t moves topic k0 + (t & 15) of rows (t >> 4) + 16 i: a row's 16 topics are 128 contiguous bytes
    const int sk = t & 15, sr = t >> 4;
    const double* tp[XV_BE / 16];
    const double* pp[XV_BW / 16];
#pragma unroll
    for (int i = 0; i < XV_BE / 16; i++) {
        const int r = e0 + sr + 16 * i;
        tp[i] = r < a.n_rows ? a.theta + (a.row_list ? (int64_t)a.row_list[r] : a.row0 + r) * K : nullptr;
    }
#pragma unroll
    for (int i = 0; i < XV_BW / 16; i++) {
        const int w = w0 + sr + 16 * i;
        pp[i] = w < a.n_types ? a.phi + (int64_t)w * K : nullptr;
    }
    double rt[XV_BE / 16], rp[XV_BW / 16];
    auto fetch = [&](int k0) {
        const int k = k0 + sk;
#pragma unroll
        for (int i = 0; i < XV_BE / 16; i++) rt[i] = (tp[i] && k < K) ? tp[i][k] : 0.0;
#pragma unroll
        for (int i = 0; i < XV_BW / 16; i++) rp[i] = (pp[i] && k < K) ? pp[i][k] : 0.0;
    };
    double acc[XV_TE][XV_TW];
#pragma unroll
    for (int i = 0; i < XV_TE; i++)
#pragma unroll
        for (int j = 0; j < XV_TW; j++) acc[i][j] = 0.0;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += XV_KS) {                    // ascending k: the order of the chain
#pragma unroll
        for (int i = 0; i < XV_BE / 16; i++) th[sk][sr + 16 * i] = rt[i];
#pragma unroll
        for (int i = 0; i < XV_BW / 16; i++) ph[sk][sr + 16 * i] = rp[i];
        __syncthreads();
        if (k0 + XV_KS < K) fetch(k0 + XV_KS);
        const int kn = K - k0;
        if (kn >= XV_KS) slab_fma<true>(th, ph, XV_KS, ty, tx, acc);
        else slab_fma<false>(th, ph, kn, ty, tx, acc);          // the topics beyond K are never multiplied
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < XV_TE; i++) {
        const int r = e0 + ty * XV_TE + i;
        if (r >= a.n_rows) continue;
        double* o = a.S + (int64_t)r * a.ldS + a.col0;
#pragma unroll
        for (int j = 0; j < XV_TW; j++) {
            const int w = w0 + 2 * tx + 16 * (j & ~1) + (j & 1);
            if (w < a.n_types) o[w] = acc[i][j];
        }
    }
}

} // namespace
