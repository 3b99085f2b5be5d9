// What parts A and B of mvtopicmodel_amd/csrc/mvhdp_side.h owe the side calls, against the stub runtime of tests/native/hip_stub: built
// with -fsanitize=address,undefined and run as a program of its own by tests/test_side_header.py.  Prints "ok" and returns 0, or names
// the first check that failed.  (Part C needs the handle and is pinned on the device by tests/test_gpu_side_preconditions.py.)
#define MVHDP_SIDE_NO_HANDLE
#include "mvhdp_side.h"
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static_assert(!std::is_copy_constructible<StreamTimer>::value && !std::is_copy_assignable<StreamTimer>::value, "StreamTimer is not copyable");

static bool is(const char* got, const char* part) { return got && strstr(got, part); }

// a call's use of the timer; leave_at: 0 runs to the end, 1 returns between start and stop, 2 before start
static int timed_call(int leave_at, double* ms)
{
    StreamTimer t;
    if (t.create() != hipSuccess) return 2;
    if (leave_at == 2) return 1;
    if (t.start(nullptr) != hipSuccess) return 3;
    if (leave_at == 1) return 1;
    g_hip.clock += 2.5f;                   // the kernels
    if (t.stop(nullptr) != hipSuccess) return 3;
    return t.elapsed_ms(ms) == hipSuccess ? 0 : 4;
}

static int lane_order(int K)
{
    const LaneTiling lt = lane_tiling(K);
    const int T = lt.T;
    CHECK(T >= 1 && T <= 32 && (T & (T - 1)) == 0);
    CHECK(64 * T >= K && (T == 1 || 64 * (T / 2) < K));                     // the smallest such power of two
    CHECK(lt.vec == (T >= 4 && K % 4 == 0));
    std::vector<int> hits((size_t)64 * T, 0);
    for (int k = 0; k < K; k++) {
        const size_t at = lane_slot(k, T);
        CHECK(at < hits.size());
        CHECK(at == (size_t)(k % T) * 64 + (size_t)(k / T));                 // entry j * 64 + lane is topic lane * T + j
        hits[at]++;
    }
    int used = 0;
    for (int v : hits) { CHECK(v <= 1); used += v; }
    CHECK(used == K);
    return 0;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // ---- check_view_weights: null, an entry, the sum -- in that order ----
    {
        const double ok2[2] = {0.25, 0.0}, one[1] = {3.0}, neg0[2] = {-0.0, 1.0};
        CHECK(check_view_weights(ok2, 2) == nullptr && check_view_weights(one, 1) == nullptr && check_view_weights(neg0, 2) == nullptr);
        CHECK(is(check_view_weights(nullptr, 2), "null"));
        const double w_nan[2] = {1.0, nan}, w_inf[2] = {inf, 1.0}, w_neg[2] = {1.0, -1e-300}, zeros[2] = {0.0, 0.0}, huge[2] = {1e308, 1e308};
        CHECK(is(check_view_weights(w_nan, 2), "negative or not finite"));
        CHECK(is(check_view_weights(w_inf, 2), "negative or not finite"));
        CHECK(is(check_view_weights(w_neg, 2), "negative or not finite"));
        CHECK(is(check_view_weights(zeros, 2), "sum"));
        CHECK(is(check_view_weights(huge, 2), "sum"));                       // every entry finite, the sum is not
        CHECK(check_view_weights(huge, 1) == nullptr);
        const double both[2] = {0.0, -1.0}, zero1[1] = {0.0};
        CHECK(is(check_view_weights(both, 2), "negative or not finite"));    // the entry is named before the sum
        CHECK(is(check_view_weights(zero1, 1), "sum"));
    }

    // ---- check_offsets: the start, then pair by pair a decrease, a span ----
    {
        const int64_t none[1] = {0}, bad0[1] = {1}, fine[4] = {0, 0, 5, 5}, from1[3] = {1, 2, 3}, dec_last[4] = {0, 2, 4, 3};
        CHECK(check_offsets(none, 0, INT64_MAX) == nullptr && check_offsets(none, 0, 0) == nullptr);
        CHECK(is(check_offsets(bad0, 0, INT64_MAX), "start at 0"));
        CHECK(check_offsets(fine, 3, INT64_MAX) == nullptr && check_offsets(fine, 3, 5) == nullptr);
        CHECK(is(check_offsets(fine, 3, 4), "span"));
        CHECK(is(check_offsets(from1, 2, INT64_MAX), "start at 0"));
        CHECK(is(check_offsets(dec_last, 3, INT64_MAX), "decreases"));
        CHECK(check_offsets(dec_last, 2, INT64_MAX) == nullptr);              // n bounds what is read
        const int64_t at_max[3] = {0, 7, 7 + (int64_t)INT32_MAX}, past_max[3] = {0, 7, 8 + (int64_t)INT32_MAX};
        CHECK(check_offsets(at_max, 2, INT32_MAX) == nullptr);
        CHECK(is(check_offsets(past_max, 2, INT32_MAX), "span"));
        CHECK(check_offsets(past_max, 2, INT64_MAX) == nullptr);
        const int64_t widest[2] = {0, INT64_MAX}, span_then_dec[4] = {0, 9, 8, 8}, dec_then_span[4] = {0, 1, 0, 9};
        CHECK(check_offsets(widest, 1, INT64_MAX) == nullptr);
        CHECK(is(check_offsets(span_then_dec, 3, 5), "span"));               // whichever pair comes first
        CHECK(is(check_offsets(dec_then_span, 3, 5), "decreases"));
    }

    // ---- check_nonneg_finite, check_tokens_nonneg ----
    {
        const double fine[3] = {0.0, -0.0, 1e308}, w_nan[2] = {1.0, nan}, w_inf[1] = {inf}, w_neg[3] = {0.0, 1.0, -4.9e-324};
        CHECK(check_nonneg_finite(fine, 3) == nullptr);                      // -0.0 passes
        CHECK(check_nonneg_finite(w_nan, 0) == nullptr && check_nonneg_finite(nullptr, 0) == nullptr);
        CHECK(check_nonneg_finite(w_nan, 1) == nullptr);
        CHECK(is(check_nonneg_finite(w_nan, 2), "negative or not finite"));
        CHECK(is(check_nonneg_finite(w_inf, 1), "negative or not finite"));
        CHECK(is(check_nonneg_finite(w_neg, 3), "negative or not finite"));
        const int32_t tok[3] = {0, INT32_MAX, -1};
        CHECK(check_tokens_nonneg(tok, 2) == nullptr && check_tokens_nonneg(nullptr, 0) == nullptr);
        CHECK(is(check_tokens_nonneg(tok, 3), "negative token"));
    }

    // ---- StreamTimer: what was created is destroyed, on every way out ----
    g_hip.reset();
    double ms = -1.0;
    CHECK(timed_call(0, &ms) == 0 && ms == 3.5);
    CHECK(g_hip.events_created == 2 && g_hip.events_destroyed == 2 && g_hip.events_recorded == 2 && g_hip.events_timed == 1);
    CHECK(timed_call(1, &ms) == 1 && g_hip.events_created == 4 && g_hip.events_destroyed == 4);      // between start and stop
    CHECK(timed_call(2, &ms) == 1 && g_hip.events_created == 6 && g_hip.events_destroyed == 6);      // before start
    g_hip.reset();
    g_hip.fail_event_create_at = 2;                                          // the second create fails: the first event is destroyed, once
    {
        StreamTimer t;
        CHECK(t.create() == hipErrorOutOfMemory);
        CHECK(g_hip.events_created == 1 && t.a != nullptr && t.b == nullptr);
    }
    CHECK(g_hip.events_created == 1 && g_hip.events_destroyed == 1);
    g_hip.reset();
    g_hip.fail_event_create_at = 1;                                          // the first one fails: nothing to destroy, no second create
    {
        StreamTimer t;
        CHECK(t.create() == hipErrorOutOfMemory && t.a == nullptr && t.b == nullptr);
    }
    CHECK(g_hip.events_created == 0 && g_hip.events_destroyed == 0 && g_hip.fail_event_create_at == 0);
    g_hip.reset();
    {                                                                        // never created: nothing destroyed
        StreamTimer t;
    }
    CHECK(g_hip.events_created == 0 && g_hip.events_destroyed == 0);
    g_hip.reset();
    {                                                                        // fold-in: one pair of events, a stretch per chunk, the times added up
        StreamTimer t;
        double total = 0.0;
        CHECK(t.create() == hipSuccess);
        for (int chunk = 0; chunk < 3; chunk++) {
            double one = 0.0;
            CHECK(t.start(nullptr) == hipSuccess);
            g_hip.clock += (float)chunk;
            CHECK(t.stop(nullptr) == hipSuccess);
            CHECK(t.elapsed_ms(&one) == hipSuccess && one == 1.0 + chunk);
            total += one;
        }
        CHECK(total == 6.0 && g_hip.events_created == 2 && g_hip.events_recorded == 6);
    }
    CHECK(g_hip.events_destroyed == 2);

    // ---- the lane order: a bijection of the topics into [0, 64 T) ----
    const int Ks[] = {1, 63, 64, 65, 2048};
    for (int K : Ks)
        if (int rc = lane_order(K)) return rc;
    CHECK(lane_tiling(64).T == 1 && lane_tiling(65).T == 2 && lane_tiling(256).T == 4 && lane_tiling(2048).T == 32);
    CHECK(lane_tiling(256).vec && !lane_tiling(254).vec && !lane_tiling(128).vec);

    // ---- dispatch_T: f once with the T asked for, never for another ----
    int calls = 0, seen = 0;
    auto f = [&](auto t) { calls++; seen = decltype(t)::value; return hipSuccess; };
    const int legal[] = {1, 2, 4, 8, 16, 32};
    for (int T : legal) {
        calls = 0; seen = 0;
        CHECK(dispatch_T(T, f) == hipSuccess && calls == 1 && seen == T);
    }
    calls = 0;
    CHECK(dispatch_T(3, f) == hipErrorInvalidValue && dispatch_T(64, f) == hipErrorInvalidValue && dispatch_T(0, f) == hipErrorInvalidValue && calls == 0);
    CHECK(dispatch_T(8, [](auto) { return hipErrorOutOfMemory; }) == hipErrorOutOfMemory);          // f's word is the call's

    // ---- grids, the queue order ----
    CHECK(wave_blocks(0, 256) == 1 && wave_blocks(5, 256) == 2 && wave_blocks((int64_t)1 << 40, 256) == 4096);
    CHECK(row_blocks(0, 256) == 1 && row_blocks(5, 256) == 5 && row_blocks((int64_t)1 << 40, 256) == 8192);
    std::vector<int32_t> order = {9, 9};
    const int64_t len[6] = {3, 7, 3, 0, 7, 5};
    order_by_length_desc(order, 6, [&](int32_t d) { return len[d]; });
    CHECK((order == std::vector<int32_t>{1, 4, 5, 0, 2, 3}));                // longest first, equal lengths in index order
    order_by_length_desc(order, 0, [&](int32_t d) { return len[d]; });
    CHECK(order.empty());

    printf("ok\n");
    return 0;
}
