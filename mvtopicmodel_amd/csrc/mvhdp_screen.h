// mvhdp_screen.h — the cosine screen that mvhdp_similar_pairs and mvhdp_nearest_entities share: the classes of a row, the rows' preparation
// (mvhdp_sim.hip holds the kernels), the 128 x 128 fp32 MFMA tile and the exact fp64 chain behind it.  The margin (mvhdp_sim.h) bounds
// |screen - exact| for ONE fp32 fma chain over the normalised image; both screen kernels run screen_tile, so they are that chain.
#pragma once
#include "mvhdp_ctx.h"
#include "mvhdp_sim.h"

enum : uint8_t { ROW_OUT = 0,                // norm 0, Inf or NaN: never pairs, never listed, lists nothing
                 ROW_TAME = 1,               // screened
                 ROW_WILD = 2 };             // a non-zero |entry| outside [2^-500, 2^500]: fp64 may under- or overflow, never screened, always a candidate

// rows [n][dim] on the device (x, filled by the caller) -> cleaned in place, norms, classes ([n + pad_rows], ROW_OUT behind n) and, with
// `image`, the fp32 image of the normalised ROW_TAME rows ([n + pad_rows][ld], zero elsewhere).  pad_rows: what the screen may read behind n.
struct ScreenRows { DevArray<double> x, norm; DevArray<uint8_t> cls; DevArray<float> xn; };
static inline int64_t screen_ld(int dim) { return ((int64_t)dim + SCREEN_BK - 1) / SCREEN_BK * SCREEN_BK; }
int mvhdp_screen_prepare_rows(mvhdp_ctx* h, ScreenRows& r, int64_t n, int dim, double min_weight, int64_t pad_rows, bool image);

constexpr int SCREEN_LDS_LD = SCREEN_BK + 4;                   // 36 floats: 16-byte aligned rows, b128 reads of a wave spread over the banks
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The tile.  A block of 256 threads computes the 128 x 128 cells of rows arow0 .. of image xa against rows brow0 .. of image xb (both
// [.][ld]).  Per k-slab of 32 the two row panels go through LDS (As, Bs: SCREEN_TILE * SCREEN_LDS_LD floats each, 16-byte aligned); wave w
// owns the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles.  v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and
// B[k = lane >> 5][j = lane & 31]; the lane's half h = lane >> 5 reads the 16 consecutive k of its half of the slab (4 x ds_read_b128 per
// panel row), so step s multiplies k = s (h = 0) and k = 16 + s (h = 1): a permutation of the slab's k order, the same for both operands
// -- still one fp32 fma chain over every k once, which is all the margin asks for.
// C/D: acc[a][b][e] is the cell of row arow0 + 64 (w >> 1) + 32 a + (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column brow0 + 64 (w & 1) + 32 b + (lane & 31).
// The images are padded with zero rows to the end of the last tile and zero columns to a multiple of 32: no bounds checks on the loads.
__device__ __forceinline__ void screen_tile(const float* xa, const float* xb, int64_t ld, int kslabs, int64_t arow0, int64_t brow0,
                                            float* As, float* Bs, f32x16 (&acc)[2][2])
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[a][b][e] = 0.0f;

    // staging: 128 rows x 8 float4 per panel, 4 per thread (named registers: an array here ends up in scratch)
    float4 ga0, ga1, ga2, ga3, gb0, gb1, gb2, gb3;
    const int srow = t >> 3, sc4 = (t & 7) * 4;                // this thread's cells of a panel: rows srow + 32 q, floats sc4 .. sc4 + 3
    const float* gpa = xa + (arow0 + srow) * ld + sc4;
    const float* gpb = xb + (brow0 + srow) * ld + sc4;
#define SCREEN_GLOAD(slab) { const int64_t ko = (int64_t)(slab) * SCREEN_BK; \
        ga0 = *(const float4*)(gpa + ko); ga1 = *(const float4*)(gpa + 32 * ld + ko); ga2 = *(const float4*)(gpa + 64 * ld + ko); ga3 = *(const float4*)(gpa + 96 * ld + ko); \
        gb0 = *(const float4*)(gpb + ko); gb1 = *(const float4*)(gpb + 32 * ld + ko); gb2 = *(const float4*)(gpb + 64 * ld + ko); gb3 = *(const float4*)(gpb + 96 * ld + ko); }
    SCREEN_GLOAD(0)
    const int lr = lane & 31, lh = lane >> 5;
    for (int slab = 0; slab < kslabs; slab++) {
        __syncthreads();                                       // the previous slab's reads are done
        {
            float* sa = As + srow * SCREEN_LDS_LD + sc4;
            float* sb = Bs + srow * SCREEN_LDS_LD + sc4;
            *(float4*)sa = ga0; *(float4*)(sa + 32 * SCREEN_LDS_LD) = ga1; *(float4*)(sa + 64 * SCREEN_LDS_LD) = ga2; *(float4*)(sa + 96 * SCREEN_LDS_LD) = ga3;
            *(float4*)sb = gb0; *(float4*)(sb + 32 * SCREEN_LDS_LD) = gb1; *(float4*)(sb + 64 * SCREEN_LDS_LD) = gb2; *(float4*)(sb + 96 * SCREEN_LDS_LD) = gb3;
        }
        __syncthreads();
        if (slab + 1 < kslabs) { SCREEN_GLOAD(slab + 1) }      // in flight under the MFMAs
        float av[2][16], bv[2][16];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 va = *(const float4*)(As + (wr + a * 32 + lr) * SCREEN_LDS_LD + lh * 16 + q * 4);
                const float4 vb = *(const float4*)(Bs + (wc + a * 32 + lr) * SCREEN_LDS_LD + lh * 16 + q * 4);
                av[a][q * 4 + 0] = va.x; av[a][q * 4 + 1] = va.y; av[a][q * 4 + 2] = va.z; av[a][q * 4 + 3] = va.w;
                bv[a][q * 4 + 0] = vb.x; bv[a][q * 4 + 1] = vb.y; bv[a][q * 4 + 2] = vb.z; bv[a][q * 4 + 3] = vb.w;
            }
#pragma unroll
        for (int s = 0; s < 16; s++) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], bv[0][s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], bv[1][s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], bv[0][s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], bv[1][s], acc[1][1], 0, 0, 0);
        }
    }
#undef SCREEN_GLOAD
}

// The exact stage's dot product: the reference's chain (SparseVector.dotProductInternal / MatrixOps.dotProduct), s = s + a[k] * b[k], dmul
// then dadd, ascending k.  Rows of even dim go two entries a load -- the same operations in the same order: a lane walks its own two rows,
// so every load instruction of the wave touches up to 64 lines whatever its width.  That path needs 16-byte aligned rows: a and b are
// rows of [.][dim] fp64 arrays that start a DevArray allocation (hipMalloc: 256-byte aligned), at i * dim * 8 bytes, a multiple of 16
// when dim is even.
__device__ __forceinline__ double screen_exact_dot(const double* a, const double* b, int dim)
{
    double s = 0.0;
    if ((dim & 1) == 0) {
        const double2* a2 = (const double2*)a;
        const double2* b2 = (const double2*)b;
#pragma unroll 4
        for (int q = 0; q < dim / 2; q++) {
            const double2 u = a2[q], v = b2[q];
            s = s + u.x * v.x;
            s = s + u.y * v.y;
        }
    } else
        for (int k = 0; k < dim; k++) s = s + a[k] * b[k];
    return s;
}
