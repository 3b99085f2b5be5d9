// mvhdp_select.h — wave-level (64-lane) device helpers of the kernels that count, compact and select: ballots, appends, order-preserving
// keys, the sorted top-n list and the bitwise descent to the n-th largest key.  Integers only; every function keeps the wave's control flow uniform.
#pragma once
#include "mvhdp_wave.h"

typedef unsigned long long u64;

__device__ __forceinline__ u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// the lanes below this one: popcount(ballot(p) & lanes_below(lane)) is the lane's place among the lanes with p
__device__ __forceinline__ u64 lanes_below(int lane) { return (1ull << lane) - 1ull; }
// the sum over the wave, as a scalar (every lane holds it after the butterfly): an atomic that adds it needs no scan over the lanes
__device__ __forceinline__ int wave_sum(int c) { for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64); return __builtin_amdgcn_readfirstlane(c); }

// One wave appends the keys of its lanes with `pass` to buf (capacity cap); *counter goes on counting beyond cap, so that the host
// learns the size a redo needs.  Wave-uniform control flow.
__device__ __forceinline__ u64 wave_append_slot(bool pass, u64* counter, int lane)
{
    const u64 m = ballot(pass);
    if (!m) return ~0ull;
    const int leader = __ffsll((long long)m) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(counter, (u64)__popcll(m));
    base = __shfl(base, leader);
    return base + (u64)__popcll(m & lanes_below(lane));
}

// order-preserving keys: a < b as numbers (no NaN) iff key(a) < key(b); -0.0 < +0.0 here.  A key is never 0 for a number.
__device__ __forceinline__ uint32_t f32_key(float v) { const uint32_t b = __float_as_uint(v); return (b >> 31) ? ~b : b | 0x80000000u; }
__device__ __forceinline__ float f32_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }
__device__ __forceinline__ u64 f64_bits_key(u64 b) { return (b >> 63) ? ~b : b | (1ull << 63); }   // of a double held as its bits
__device__ __forceinline__ u64 f64_key(double v) { return f64_bits_key((u64)__double_as_longlong(v)); }
__device__ __forceinline__ double f64_unkey(u64 k) { return __longlong_as_double((long long)((k >> 63) ? k ^ (1ull << 63) : ~k)); }

// The sorted top-n list of a wave: lane i holds the i-th entry so far (n <= 64; the lanes from n on hold the list's tail, which nothing
// reads).  topn_offer enters the lanes' keys that come before the n-th entry `thr`, one per turn: a ballot finds the place, a shuffle
// makes the room.  before(a, b) is a strict total order on the real entries, with the empty entry after every real one and not before
// itself; an entry type of a kernel's own brings its lane_get / lane_up1 along.  Wave-uniform control flow.
__device__ __forceinline__ u64 lane_get(const u64& v, int j) { return __shfl(v, j, WAVE); }
__device__ __forceinline__ u64 lane_up1(const u64& v) { return __shfl_up(v, 1, WAVE); }
struct KeyDescending { __device__ __forceinline__ bool operator()(u64 a, u64 b) const { return a > b; } };   // u64 keys, larger first; 0 is the empty entry

template <class E, class Before>
__device__ __forceinline__ void topn_offer(E& list, E& thr, E key, int n, int lane, Before before)
{
    u64 cand = ballot(before(key, thr));
    while (cand) {
        const int j = __ffsll((long long)cand) - 1;
        const E x = lane_get(key, j);
        const int pos = __popcll(ballot(before(list, x)));
        const E up = lane_up1(list);
        if (lane == pos) list = x; else if (lane > pos) list = up;
        thr = lane_get(list, n - 1);
        cand &= (j == 63) ? 0ull : ~((2ull << j) - 1);
        cand &= ballot(before(key, thr));
    }
}

// The bitwise descent: bits top_bit .. 0 of T, from the top, are set wherever reach(T | bit) holds.  With reach(t) = "at least n keys
// are >= t" (wave-uniform) and those bits of T clear, this is the largest such value that at least n keys reach: the n-th largest key.
template <class U, class Reach>
__device__ __forceinline__ U key_descent(U T, int top_bit, Reach&& reach)
{
    for (int bit = top_bit; bit >= 0; bit--) {
        const U trial = T | ((U)1 << bit);
        if (reach(trial)) T = trial;
    }
    return T;
}
