// slim_row_gather.hip — the bare gather of row_gather_ceiling.hip over the two narrow images of n_wk side by side: does a row of the
// 12-bit image (mvhdp_slim.h: 85 cells per 128-byte line, line-aligned rows, 2-byte loads at odd addresses among them) deliver the
// lines it saves over a row of the 16-bit mirror (2K bytes, rows back to back)?
//
// As there: 7 waves per SIMD do nothing else, every wave reads `iters` random rows, two rows in flight, `used` sorted cells of a row per
// gather (a lane a cell).  Reported per image: rows per second, the 128-byte lines a row's gather touches, and their product.  The
// 12-bit gather includes the extraction (shift and mask), so that its result is the cell's value.
//   hipcc --offload-arch=gfx950 -O3 -I../../mvtopicmodel_amd/csrc -o slim_row_gather slim_row_gather.hip && ./slim_row_gather [K rows used]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <set>
#include <vector>
#include "mvhdp_slim.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef unsigned short u16_any __attribute__((aligned(1)));

// SLIM: `off` = byte offset << 5 | shift of the lane's cell inside a 12-bit row; else the byte offset inside a 16-bit row
template <bool SLIM>
__global__ __launch_bounds__(256, 7) void gather_kernel(const unsigned char* __restrict__ table, int rows, unsigned int row_bytes, const unsigned int* __restrict__ offs,
                                                        int iters, unsigned long long* out)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned int off = offs[(size_t)wave * 64 + lane];
    unsigned int rs = 0x9E3779B9u * (wave + 1);
    unsigned long long acc = 0;
    for (int it = 0; it < iters; it += 2) {
        rs = rs * 1664525u + 1013904223u;
        const size_t r0 = (size_t)(rs >> 8) % (size_t)rows;
        rs = rs * 1664525u + 1013904223u;
        const size_t r1 = (size_t)(rs >> 8) % (size_t)rows;
        unsigned int a, b;
        if (SLIM) {
            a = *(const u16_any*)(table + r0 * row_bytes + (off >> 5));
            b = *(const u16_any*)(table + r1 * row_bytes + (off >> 5));
            a = __builtin_amdgcn_ubfe(a, off, 12u);                        // (reads bits 4:0 of its offset operand)
            b = __builtin_amdgcn_ubfe(b, off, 12u);
        } else {
            a = *(const unsigned short*)(table + r0 * row_bytes + off);
            b = *(const unsigned short*)(table + r1 * row_bytes + off);
        }
        acc += a + b;
    }
    if (acc == 0x7fffffffffffULL) out[0] = acc;
}

template <bool SLIM>
static double run(const unsigned char* t, int rows, unsigned int row_bytes, const unsigned int* doffs, int waves, int iters)
{
    unsigned long long* out; CK(hipMalloc(&out, 16));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    hipLaunchKernelGGL((gather_kernel<SLIM>), dim3(waves / 4), dim3(256), 0, 0, t, rows, row_bytes, doffs, iters / 4, out);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(a));
    hipLaunchKernelGGL((gather_kernel<SLIM>), dim3(waves / 4), dim3(256), 0, 0, t, rows, row_bytes, doffs, iters, out);
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    CK(hipFree(out));
    return (double)waves * iters / (ms * 1e-3);
}

int main(int argc, char** argv)
{
    const int K = argc > 1 ? atoi(argv[1]) : 400, rows = argc > 2 ? atoi(argv[2]) : 60000, used = std::min(64, std::min(K, argc > 3 ? atoi(argv[3]) : 45));
    const int waves = 256 * 4 * 7, iters = 4000;
    const unsigned int rb16 = 2u * K, rb12 = (unsigned int)mvhdp_slim_row_bytes(K);
    unsigned char *t16, *t12;
    CK(hipMalloc(&t16, (size_t)rows * rb16 + 256)); CK(hipMemset(t16, 1, (size_t)rows * rb16));
    CK(hipMalloc(&t12, (size_t)rows * rb12 + 256)); CK(hipMemset(t12, 1, (size_t)rows * rb12));
    std::mt19937 g(1);
    std::vector<unsigned int> o16((size_t)waves * 64), o12((size_t)waves * 64);
    double lines16 = 0, lines12 = 0, odd = 0;
    for (int w = 0; w < waves; w++) {
        std::vector<int> all(K); for (int i = 0; i < K; i++) all[i] = i;
        std::shuffle(all.begin(), all.end(), g);
        std::sort(all.begin(), all.begin() + used);
        for (int i = 0; i < 64; i++) {
            const int k = all[std::min(i, used - 1)];
            o16[(size_t)w * 64 + i] = 2u * k;
            o12[(size_t)w * 64 + i] = (mvhdp_slim_byte(k) << 5) | mvhdp_slim_shift(k);
            if (i < used && (mvhdp_slim_byte(k) & 1u)) odd += 1;
        }
        // distinct 128-byte lines of the gather: the 16-bit row averaged over the alignments a row of 2K bytes can have, the 12-bit row line-aligned
        const int phases = 128 / std::gcd(128, (2 * K) % 128 ? (2 * K) % 128 : 128);
        double l = 0;
        for (int ph = 0; ph < phases; ph++) {
            const int off = (ph * 2 * K) % 128;
            std::set<int> s;
            for (int i = 0; i < used; i++) s.insert((off + 2 * all[i]) / 128);
            l += (double)s.size();
        }
        lines16 += l / phases;
        std::set<int> s;
        for (int i = 0; i < used; i++) s.insert(all[i] / MVHDP_SLIM_CELLS);
        lines12 += (double)s.size();
    }
    lines16 /= waves; lines12 /= waves; odd /= (double)waves * used;
    unsigned int *d16, *d12;
    CK(hipMalloc(&d16, o16.size() * 4)); CK(hipMemcpy(d16, o16.data(), o16.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&d12, o12.size() * 4)); CK(hipMemcpy(d12, o12.data(), o12.size() * 4, hipMemcpyHostToDevice));
    const double r16 = run<false>(t16, rows, rb16, d16, waves, iters), r12 = run<true>(t12, rows, rb12, d12, waves, iters);
    const double r16b = run<false>(t16, rows, rb16, d16, waves, iters), r12b = run<true>(t12, rows, rb12, d12, waves, iters);
    printf("K = %d, %d rows, %d waves (7 per SIMD), %d cells of a row per gather; %.2f of the 12-bit cells start at an odd address\n", K, rows, waves, used, odd);
    printf("16-bit rows of %4u B (%5.1f MB): %7.3f / %7.3f G rows/s x %5.2f lines x 128 B = %7.1f GB/s of fabric reads\n", rb16, rows * (double)rb16 / 1e6, r16 / 1e9, r16b / 1e9, lines16, r16b * lines16 * 128 / 1e9);
    printf("12-bit rows of %4u B (%5.1f MB): %7.3f / %7.3f G rows/s x %5.2f lines x 128 B = %7.1f GB/s of fabric reads\n", rb12, rows * (double)rb12 / 1e6, r12 / 1e9, r12b / 1e9, lines12, r12b * lines12 * 128 / 1e9);
    printf("rows per second, 12-bit over 16-bit: %.3f (lines: %.3f)\n", r12b / r16b, lines16 / lines12);
    return 0;
}
