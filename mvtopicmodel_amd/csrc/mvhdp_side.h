// mvhdp_side.h — the host side that the side calls on a trained handle share (diagnostics, similarity, nearest entities, cross-view
// prediction either way, held-out likelihood, fold-in, topic Gram, cohort words, word co-occurrence, topic remap, topic split): the argument checks, the call prologue, the stream
// timer, the grid sizes and the lane-order choreography of the one-wave-per-document kernels.  Host code only; no kernel lives here.
#pragma once
#include <cmath>
#include <cstdint>
#include <climits>

// ---- Part A: pure checkers, no handle and no HIP.  Each returns nullptr when the argument is fine, else the reason as the tail of a
// message; the entry puts its own name and the argument's in front: FAIL(h, code, who + ": q_off " + reason). ----
// w [M]: null; an entry negative or not finite; the sum not positive or not finite -- in that order
inline const char* check_view_weights(const double* w, int M)
{
    if (!w) return "null view_weights";
    double sum = 0.0;
    for (int m = 0; m < M; m++) {
        if (!(w[m] >= 0.0) || !std::isfinite(w[m])) return "a view weight is negative or not finite";
        sum += w[m];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return "the view weights do not sum to a positive finite number";
    return nullptr;
}

// off [n + 1], CSR offsets: off[0] != 0; then pair by pair a decrease, a span above max_span (INT64_MAX: no limit)
inline const char* check_offsets(const int64_t* off, int64_t n, int64_t max_span)
{
    if (off[0] != 0) return "does not start at 0";
    for (int64_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return "decreases";
        if (off[i + 1] - off[i] > max_span) return "has a span above the limit";
    }
    return nullptr;
}

// x [n]: -0.0 passes, NaN does not
inline const char* check_nonneg_finite(const double* x, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (!(x[i] >= 0.0) || !std::isfinite(x[i])) return "is negative or not finite";
    return nullptr;
}

inline const char* check_tokens_nonneg(const int32_t* tok, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (tok[i] < 0) return "negative token";
    return nullptr;
}

// ---- Part B: what needs the HIP runtime or the standard library only ----
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include <vector>

// The time between two points of a stream (a call's kernel_ms).  create() once; start / stop / elapsed_ms as often as the call has
// stretches to time (fold-in: one per chunk), elapsed_ms after the stream has passed stop.  Whatever was created is destroyed on every
// way out of the scope.
struct StreamTimer {
    hipEvent_t a = nullptr, b = nullptr;
    StreamTimer() = default;
    StreamTimer(const StreamTimer&) = delete;
    StreamTimer& operator=(const StreamTimer&) = delete;
    ~StreamTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t create() { const hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }   // a failed create leaves its event null
    hipError_t start(hipStream_t s) { return hipEventRecord(a, s); }
    hipError_t stop(hipStream_t s) { return hipEventRecord(b, s); }
    hipError_t elapsed_ms(double* ms)
    {
        float f = 0.0f;
        const hipError_t e = hipEventElapsedTime(&f, a, b);
        *ms = (double)f;
        return e;
    }
};

// grids of the one-wave-per-item kernels (four waves a block) and of the one-block-per-row kernels
inline unsigned wave_blocks(int64_t waves, int num_cus) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)num_cus * 16)); }
inline unsigned row_blocks(int64_t rows, int num_cus) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)num_cus * 32)); }

// The lane order of heldout_ltr_kernel and foldin_kernel: lane l owns the T topics l T .. l T + T - 1, T the smallest power of two with
// 64 T >= K; vec: a lane's cells of a count row go in 16-byte loads.  Topic k sits at entry lane_slot(k, T) of a [64 T] table.
struct LaneTiling { int T; bool vec; };
inline LaneTiling lane_tiling(int K)
{
    int T = 1;
    while (64 * T < K) T <<= 1;
    return { T, T >= 4 && K % 4 == 0 };
}
inline size_t lane_slot(int k, int T) { return (size_t)(k % T) * 64 + (size_t)(k / T); }

// f(std::integral_constant<int, T>) for T = 1, 2, 4, .. 32: the launch of a kernel templated on T
template <class F> hipError_t dispatch_T(int T, F&& f)
{
    switch (T) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    }
    return hipErrorInvalidValue;
}

// order = 0 .. n - 1 by len(i) descending, equal lengths in index order: the queue order of a chunk's documents, longest first
template <class Len> void order_by_length_desc(std::vector<int32_t>& order, int64_t n, Len len)
{
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t l, int32_t r) { return len(l) > len(r); });
}

// ---- Part C: what needs the handle.  The CPU probe (tests/native/side_probe.cpp) defines MVHDP_SIDE_NO_HANDLE to build parts A and B
// with the host compiler against a stub runtime. ----
#ifndef MVHDP_SIDE_NO_HANDLE
#include "mvhdp_ctx.h"

// the counts hold every assignment and no NO_APPLY sweep's deltas wait beside them: "not current" before "pending"
inline int require_current_counts(mvhdp_ctx* h, const std::string& who)
{
    if (!h->st.have_counts() || h->st.counts_stale()) FAIL(h, MVHDP_ERR_STATE, who + ": the counts are not current (build_counts / set_counts first)");
    if (h->st.delta_pending()) FAIL(h, MVHDP_ERR_STATE, who + ": a NO_APPLY sweep's deltas are pending (mvhdp_apply_delta first)");
    return MVHDP_OK;
}

// the prologue of a call that reads what the handle's stream may still be writing
inline int side_begin(mvhdp_ctx* h)
{
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));                  // what is pending on the handle lands first
    return MVHDP_OK;
}
#endif
