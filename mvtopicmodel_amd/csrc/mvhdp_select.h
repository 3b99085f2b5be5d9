// mvhdp_select.h — wave-level (64-lane) device helpers of the kernels that count, compact and select: ballots, appends, order-preserving
// keys, the sorted top-n list, the bitwise descent to the n-th largest key, the first n entries of a row in order (wave_first_n) and the
// count of the entries that precede one (wave_rank_count).  Integers only; every function keeps the wave's control flow uniform.
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
// The two on bits are the host's as well: a list of keys that comes back from the device is turned into doubles there.
__host__ __device__ __forceinline__ u64 f64_bits_key(u64 b) { return (b >> 63) ? ~b : b | (1ull << 63); }   // of a double held as its bits
__host__ __device__ __forceinline__ u64 f64_key_bits(u64 k) { return (k >> 63) ? k ^ (1ull << 63) : ~k; }   // ... and back
__device__ __forceinline__ u64 f64_key(double v) { return f64_bits_key((u64)__double_as_longlong(v)); }
__device__ __forceinline__ double f64_unkey(u64 k) { return __longlong_as_double((long long)f64_key_bits(k)); }

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

// The first n of a row, in order.  Of m entries, entry i the composite (hi, lo) = at(i, hi, lo) with hi == 0 for an entry that does not
// count, the n_eff = min(n_cap, entries that count) largest composites (hi first, then lo; the composites that count are distinct), in
// descending order: emit(place, hi, lo).  sel_hi / sel_lo: [n_cap] scratch of this wave in memory.  Returns n_eff.  The block is this
// one wave (__syncthreads is where the wave reads what its other lanes wrote).  The row is read once for the count and the bits every
// key shares, once per bit below them that the keys do not share, and 32 times more only where equal keys straddle the n-th place.
template <class I, class At, class Emit>
__device__ __forceinline__ int wave_first_n(At&& at, I m, int n_cap, int lane, u64* sel_hi, uint32_t* sel_lo, Emit&& emit)
{
    const u64 below = lanes_below(lane);
    // how many entries pass the test: every lane counts its own (i = lane, lane + 64, ..), the 64 counts are added at the end.  Every
    // test below is against a threshold that is not 0, so an entry that does not count never passes.
    auto count = [&](auto&& test) -> int {
        int c = 0;
#pragma unroll 8
        for (I i = lane; i < m; i += 64) { u64 h; uint32_t l; at(i, h, l); c += test(h, l) ? 1 : 0; }
        return wave_sum(c);
    };
    int nv = 0;
    u64 all_and = ~0ull, all_or = 0;
#pragma unroll 8
    for (I i = lane; i < m; i += 64) {
        u64 h; uint32_t l; at(i, h, l);
        if (h != 0) { nv++; all_and &= h; all_or |= h; }
    }
    for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); all_and &= __shfl_xor(all_and, o, 64); all_or |= __shfl_xor(all_or, o, 64); }   // one butterfly for the three
    nv = __builtin_amdgcn_readfirstlane(nv);
    const int n_eff = nv < n_cap ? nv : n_cap;
    if (n_eff == 0) return 0;
    u64 th = 0; uint32_t tl = 0;                               // the n_eff-th composite; (0, 0) takes every entry that counts
    if (nv > n_eff) {
        // the largest key that at least n_eff keys reach (a key of the row, so not 0); the bits every key shares are settled
        const u64 diff = all_and ^ all_or;
        th = all_and;
        if (diff) {
            const int hb = 63 - __builtin_clzll(diff);
            th = key_descent(hb == 63 ? 0ull : all_and & ~((2ull << hb) - 1), hb, [&](u64 trial) { return count([&](u64 h, uint32_t) { return h >= trial; }) >= n_eff; });
        }
        // equal keys across the n-th place: lo decides
        if (!diff || count([&](u64 h, uint32_t) { return h >= th; }) > n_eff)
            tl = key_descent(0u, 31, [&](uint32_t trial) { return count([&](u64 h, uint32_t l) { return h > th || (h == th && l >= trial); }) >= n_eff; });
    }
    int got = 0;
    for (I base = 0; base < m; base += 64) {
        const I i = base + lane;
        u64 h = 0; uint32_t l = 0;
        if (i < m) at(i, h, l);
        const bool sel = h != 0 && (h > th || (h == th && l >= tl));
        const u64 mk = ballot(sel);
        if (sel) { const int pos = got + __popcll(mk & below); sel_hi[pos] = h; sel_lo[pos] = l; }   // pos < n_eff: exactly n_eff entries pass
        got += __popcll(mk);
    }
    __syncthreads();                                           // the wave reads what its other lanes wrote
    // each kept entry goes to the place given by the number in front of it: a lane holds one entry of a run of 64 and counts, run by
    // run, the entries of the other lanes as they are broadcast (one coalesced read a run, no trip to memory per comparison)
    for (int i0 = 0; i0 < n_eff; i0 += 64) {
        const int i = i0 + lane;
        u64 h = 0; uint32_t l = 0;
        if (i < n_eff) { h = sel_hi[i]; l = sel_lo[i]; }
        int place = 0;
        for (int j0 = 0; j0 < n_eff; j0 += 64) {
            u64 hj = h; uint32_t lj = l;
            if (j0 != i0 && j0 + lane < n_eff) { hj = sel_hi[j0 + lane]; lj = sel_lo[j0 + lane]; }
            const int nj = n_eff - j0 < 64 ? n_eff - j0 : 64;
            for (int s = 0; s < nj; s++) {
                const u64 bh = ((u64)(uint32_t)bcast_i((int)(hj >> 32), s) << 32) | (u64)(uint32_t)bcast_i((int)(uint32_t)hj, s);
                const uint32_t bl = (uint32_t)bcast_i((int)lj, s);
                place += (bh > h || (bh == h && bl > l)) ? 1 : 0;
            }
        }
        if (i < n_eff) emit(place, h, l);
    }
    return n_eff;
}

// The rank of one entry in its row: of the n cells of `row` (scores held as bits; cell w has the id id0 + w), how many count (key not
// 0), are not the queried id q and precede (kq, q): a larger key, or the same key and a smaller id.  One wave; returns the wave's count.
__device__ __forceinline__ int wave_rank_count(const u64* __restrict__ row, int n, uint32_t id0, u64 kq, uint32_t q, int lane)
{
    int c = 0;
    for (int w = lane; w < n; w += 64) {
        const u64 key = f64_bits_key(row[w]);
        const uint32_t id = id0 + (uint32_t)w;
        c += (key != 0 && id != q && (key > kq || (key == kq && id < q))) ? 1 : 0;
    }
    return wave_sum(c);
}
