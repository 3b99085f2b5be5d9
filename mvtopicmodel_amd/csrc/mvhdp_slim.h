// mvhdp_slim.h — the 12-bit image of n_wk (MvModel::counts12): layout of a row, one definition for the pass that writes it
// (mvhdp_kernels.hip), the kernels that gather from it (mvhdp_sweep_fast.hip), the bare-gather microbenchmark and the CPU test.
//
//   rows are 128-byte aligned; line j of a row holds cells 85*j .. 85*j + 84, little-endian, two cells per three bytes
//   (85 cells = 127.5 bytes: no cell crosses a line); a row has ceil(K / 85) lines -- 5 at K = 400 (a 16-bit row of 800 bytes spans 7),
//   12 at K = 1000 (against 16); bytes no cell uses are zero.
//   cell k: the 16 bits at byte offset 128 * (k / 85) + ((3 * (k % 85)) >> 1), shifted right by 4 * ((k % 85) & 1), low 12 bits.
// A row is in this image for a sweep (a "slim" row, MVHDP_ROW_SLIM) when every cell of the sweep's snapshot is at most 4095.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVHDP_SLIM_FN __host__ __device__ static inline
#else
#define MVHDP_SLIM_FN static inline
#endif

enum { MVHDP_SLIM_LINE = 128, MVHDP_SLIM_CELLS = 85, MVHDP_SLIM_MAX = 4095 };

// bytes of a row (its stride: rows follow each other line-aligned)
MVHDP_SLIM_FN size_t mvhdp_slim_row_bytes(int K) { return (size_t)MVHDP_SLIM_LINE * (size_t)((K + MVHDP_SLIM_CELLS - 1) / MVHDP_SLIM_CELLS); }
// byte offset, inside its row, of the two bytes that hold cell k
MVHDP_SLIM_FN unsigned int mvhdp_slim_byte(int k) { const unsigned int j = (unsigned int)k / MVHDP_SLIM_CELLS, i = (unsigned int)k - j * MVHDP_SLIM_CELLS; return MVHDP_SLIM_LINE * j + ((3u * i) >> 1); }
// ... and the shift that brings the cell to bit 0 of those 16 bits
MVHDP_SLIM_FN unsigned int mvhdp_slim_shift(int k) { return 4u * (((unsigned int)k % MVHDP_SLIM_CELLS) & 1u); }

// (host and device; the two bytes may sit at an odd address)
MVHDP_SLIM_FN unsigned int mvhdp_slim_get(const unsigned char* row, int k)
{
    const unsigned char* p = row + mvhdp_slim_byte(k);
    return ((((unsigned int)p[1] << 8) | (unsigned int)p[0]) >> mvhdp_slim_shift(k)) & 0xfffu;
}
// v <= 4095, into a row whose cell k is still zero
MVHDP_SLIM_FN void mvhdp_slim_put(unsigned char* row, int k, unsigned int v)
{
    unsigned char* p = row + mvhdp_slim_byte(k);
    const unsigned int w = (v & 0xfffu) << mvhdp_slim_shift(k);
    p[0] = (unsigned char)(p[0] | (w & 0xffu));
    p[1] = (unsigned char)(p[1] | (w >> 8));
}

// Whether the image can pay for a model of K topics whose largest view has max_types types: its rows must have fewer lines than the rows of
// the 16-bit mirror span at the least (ceil(K / 64)), and the type ids must leave bit 28 free for the row's class (W_SLIM of the sweep kernel;
// the library accepts views of up to 2^29 - 1 types, and those keep the mirror).  level: 0 never; 1 where a row is long enough for its lines to
// be what a sweep is bound by (K >= 256, as for the mirror itself); 2 wherever the lines are fewer (measurements).
MVHDP_SLIM_FN int mvhdp_slim_pays(int K, int max_types, int level)
{
    if (level == 0 || max_types >= (1 << 28)) return 0;
    if ((K + MVHDP_SLIM_CELLS - 1) / MVHDP_SLIM_CELLS >= (K + 63) / 64) return 0;
    return (level >= 2 || K >= 256) ? 1 : 0;
}
