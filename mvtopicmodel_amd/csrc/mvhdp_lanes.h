// mvhdp_lanes.h — topics owned by lanes: the pieces the one-wave-per-document kernels share (heldout_ltr_kernel in mvhdp_heldout.hip,
// foldin_kernel in mvhdp_foldin.hip).  Lane l of the wave owns the T topics l T .. l T + T - 1 (T = 1, 2, 4, .. 32, the smallest with
// 64 T >= K); include/mvhdp.h (the summation-order paragraph of mvhdp_heldout_left_to_right) fixes what a draw over such weights is.
#pragma once
#include "mvhdp_wave.h"

// a 64-bit value the compiler must treat as wave-uniform (it is: lane 0's)
__device__ __forceinline__ int64_t uniform_i64(int64_t x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)x >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// the count cells of lane's T topics of row w; cells beyond K read as 0
template <int T, bool VEC>
__device__ __forceinline__ void gather_row(const int32_t* __restrict__ rows, int w, int K, int lane, int (&row)[T])
{
    const int32_t* __restrict__ rp = rows + (int64_t)w * K;
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < T; j += 4) {
            const int k = lane * T + j;
            int4 v = make_int4(0, 0, 0, 0);
            if (k < K) v = *reinterpret_cast<const int4*>(rp + k);    // K % 4 == 0: the four cells are inside the row together, 16-byte aligned
            row[j] = v.x; row[j + 1] = v.y; row[j + 2] = v.z; row[j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int k = lane * T + j;
            row[j] = k < K ? rp[k] : 0;
        }
    }
}

// The draw: excl = the scanned lane sums of the lanes below (0.0 in lane 0), target = u * total.  Every lane searches its own topics for the
// first with wt > 0.0 whose running sum excl + pre exceeds target; a ballot names the first lane that found one; if none did, the last topic
// with wt > 0.0 (topic 0 if every weight is 0).  The topic is sel_lane * T + sel_j, both wave-uniform.  (heldout_ltr_kernel keeps these
// lines written out in its visit: calling this function there instead changes that kernel's register allocation, and its listing is to
// stay as it is; with uniform_i64 and gather_row taken from here its listing is unchanged.)
template <int T>
__device__ __forceinline__ void lane_draw(const double (&wt)[T], double excl, double target, int& sel_lane, int& sel_j)
{
    int cand = -1, last = -1;
    double pre = 0.0;
#pragma unroll
    for (int j = 0; j < T; j++) {
        pre = j == 0 ? wt[0] : pre + wt[j];
        if (wt[j] > 0.0) {
            last = j;
            if (cand < 0 && excl + pre > target) cand = j;
        }
    }
    sel_lane = 0; sel_j = 0;
    const unsigned long long found = __builtin_amdgcn_ballot_w64(cand >= 0);
    if (found) {
        sel_lane = __builtin_ctzll(found);
        sel_j = bcast_i(cand, sel_lane);
    } else {
        const unsigned long long any = __builtin_amdgcn_ballot_w64(last >= 0);
        if (any) {
            sel_lane = 63 - __builtin_clzll(any);
            sel_j = bcast_i(last, sel_lane);
        }
    }
}
