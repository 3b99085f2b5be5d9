// mvhdp_remap.hip — mvhdp_remap_topics: merge, drop and reorder topics on the trained handle (include/mvhdp.h has the contract).  One
// topic map [K] is applied, one hop, to the assignments, the counts, alpha and the inactive set together; the handle is left as
// mvhdp_set_assignments of every view followed by mvhdp_build_counts would leave it.  Integers only on the device.
//   remap_z_kernel        over one view's z: the map in LDS, 16-byte loads and stores with an unaligned head and tail done by scalars, a
//                         lane stores only where one of its topics changed; moved / dropped by ballot and popcount per wave, one atomic
//                         per block and counter.
//   remap_fold_kernel<T>  over the sumV + M rows of MVHDP_BUF_COUNTS (the n_k rows are rows like any other): one wave per row, four a
//                         block, lane l owns the cells l, l + 64, ..; the row is read whole into registers before anything of it is
//                         written (a cyclic map is safe in place), added at map[k] into the wave's LDS slice, and written back where a
//                         cell changed.  A row that is all zero -- most rows of a sparse table are nearly so -- skips the LDS round trip.
// The alpha / inactive fold is K-sized and stays on the host, as apply_activation does.
#include "mvhdp_side.h"
#include "mvhdp_select.h"

namespace {

__global__ __launch_bounds__(256) void remap_z_kernel(int32_t* __restrict__ z, int64_t n, const int32_t* __restrict__ map, int K, u64* __restrict__ ctr /*[2] moved, dropped*/)
{
    __shared__ int32_t smap[MVHDP_MAX_TOPICS];
    __shared__ unsigned int blk[2];
    for (int k = threadIdx.x; k < K; k += blockDim.x) smap[k] = map[k];
    if (threadIdx.x < 2) blk[threadIdx.x] = 0;
    __syncthreads();
    // a topic outside [0, K) -- unassigned, or not a topic at all -- stays what it is
    auto hop = [&](int t) { return (unsigned)t < (unsigned)K ? smap[t] : t; };
    unsigned int moved = 0, dropped = 0;                       // wave-uniform
    auto count = [&](int o, int t) {
        moved += (unsigned)__popcll(ballot(t != o && t >= 0));
        dropped += (unsigned)__popcll(ballot(t != o && t < 0));
    };
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    const int64_t lead = (int64_t)((16 - ((uintptr_t)z & 15)) & 15) / 4, head = lead < n ? lead : n;   // tokens in front of the first 16-byte border
    const int64_t nvec = (n - head) / 4, tail = head + nvec * 4;
    int4* zv = (int4*)(z + head);
    // every wave makes the same number of trips (the ballots need whole waves): the bound is rounded up to a wave
    for (int64_t i = tid; i < ((nvec + WAVE - 1) & ~(int64_t)(WAVE - 1)); i += nthreads) {
        const bool in = i < nvec;
        int4 o = in ? zv[i] : make_int4(-1, -1, -1, -1), t;
        t.x = hop(o.x); t.y = hop(o.y); t.z = hop(o.z); t.w = hop(o.w);
        count(o.x, t.x); count(o.y, t.y); count(o.z, t.z); count(o.w, t.w);
        if (in && (t.x != o.x || t.y != o.y || t.z != o.z || t.w != o.w)) zv[i] = t;
    }
    // the head and the tail: at most three tokens each, the first wave's
    if (tid < WAVE) {
        const int64_t i = tid < head ? tid : tail + (tid - head);
        const bool in = tid < head || i < n;
        const int o = in ? z[i] : -1, t = hop(o);
        count(o, t);
        if (in && t != o) z[i] = t;
    }
    if ((threadIdx.x & 63) == 0) {
        if (moved) atomicAdd(&blk[0], moved);
        if (dropped) atomicAdd(&blk[1], dropped);
    }
    __syncthreads();
    if (threadIdx.x < 2 && blk[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (u64)blk[threadIdx.x]);
}

template <int T>
__global__ __launch_bounds__(256) void remap_fold_kernel(int32_t* __restrict__ counts, int64_t nrows, const int32_t* __restrict__ map, int K)
{
    extern __shared__ int32_t fold_lds[];                      // [K] the map, then [4][K] a slice per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* smap = fold_lds;
    int32_t* acc = fold_lds + (size_t)(1 + wave) * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) smap[k] = map[k];
    __syncthreads();
    int dst[T];                                                // where this lane's cells go: -1 nowhere
#pragma unroll
    for (int j = 0; j < T; j++) { const int k = lane + j * WAVE; dst[j] = k < K ? smap[k] : -1; }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < nrows; row += (int64_t)gridDim.x * 4) {
        int32_t* r = counts + row * K;
        int c[T];
        bool any = false;
#pragma unroll
        for (int j = 0; j < T; j++) { const int k = lane + j * WAVE; c[j] = k < K ? r[k] : 0; any = any || c[j] != 0; }
        if (!ballot(any)) continue;                            // nothing to move, nothing to write
#pragma unroll
        for (int j = 0; j < T; j++) { const int k = lane + j * WAVE; if (k < K) acc[k] = 0; }
        LDS_FENCE();
#pragma unroll
        for (int j = 0; j < T; j++) if (c[j] != 0 && dst[j] >= 0) atomicAdd(&acc[dst[j]], c[j]);
        LDS_FENCE();
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int k = lane + j * WAVE;
            if (k < K) { const int v = acc[k]; if (v != c[j]) r[k] = v; }
        }
        LDS_FENCE();
    }
}

enum { REMAP_LDS_ROWS = 5 };                                   // the map and four slices

// the K-sized part of the call, all on the host: what alpha and the inactive set become, and what the statistics say of the topics
struct TopicFold {
    std::vector<double> alpha;                                 // [M][K + 1]
    std::vector<uint8_t> inactive;                             // [K]
    int32_t vacated = 0, retired = 0;
    bool drops[MVHDP_MAXM] = {};                               // a dropped topic held tokens of the view
};

void fold_topics(const mvhdp_ctx* h, const int32_t* map, uint32_t flags, const std::vector<int32_t>& nk /*[M][K]*/, TopicFold& f)
{
    const int K = h->mm.K, M = h->mm.M;
    std::vector<int32_t> sources((size_t)K, 0);
    f.alpha = h->h_alpha;
    f.inactive.assign((size_t)K, 1);
    for (int m = 0; m < M; m++) for (int t = 0; t < K; t++) f.alpha[(size_t)m * (K + 1) + t] = 0.0;
    for (int k = 0; k < K; k++) {                              // ascending k: the order of the sums
        const int t = map[k];
        if (t < 0) { for (int m = 0; m < M; m++) f.drops[m] = f.drops[m] || nk[(size_t)m * K + k] > 0; continue; }
        for (int m = 0; m < M; m++) {
            double& a = f.alpha[(size_t)m * (K + 1) + t];
            const double add = h->h_alpha[(size_t)m * (K + 1) + k];
            if (sources[(size_t)t] == 0) a = add; else a = a + add;          // a single source moves its bits
        }
        f.inactive[(size_t)t] = f.inactive[(size_t)t] && h->h_inactive[(size_t)k];
        sources[(size_t)t]++;
    }
    for (int t = 0; t < K; t++) {
        if (sources[(size_t)t]) continue;
        bool held = false;
        for (int m = 0; m < M; m++) held = held || nk[(size_t)m * K + t] > 0;
        f.inactive[(size_t)t] = h->h_inactive[(size_t)t] || (flags & MVHDP_REMAP_RETIRE) != 0;
        if (held || !h->h_inactive[(size_t)t]) { f.vacated++; if (f.inactive[(size_t)t]) f.retired++; }
    }
}

int remap_run(mvhdp_ctx* h, const mvhdp_remap_args* a, mvhdp_remap_stats& st)
{
    MvModel& mm = h->mm;
    const int K = mm.K, M = mm.M;
    const int64_t nrows = mm.rowbase[M] + M;
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    std::vector<int32_t> nk((size_t)M * K);
    HIPC(h, hipMemcpyAsync(nk.data(), mm.counts + mm.rowbase[M] * K, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    TopicFold f;
    fold_topics(h, a->map, a->flags, nk, f);

    // everything that can fail without a kernel having run comes first
    DevArray<int32_t> d_map;
    DevArray<u64> d_ctr;
    HIPC(h, d_map.alloc((size_t)K));
    HIPC(h, d_ctr.alloc((size_t)2 * MVHDP_MAXM));
    const size_t lds = (size_t)REMAP_LDS_ROWS * K * sizeof(int32_t);
    const LaneTiling lt = lane_tiling(K);
    HIPC(h, dispatch_T(lt.T, [&](auto t) { return hipFuncSetAttribute((const void*)remap_fold_kernel<decltype(t)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }));
    StreamTimer timer;
    HIPC(h, timer.create());
    const std::vector<long long> none((size_t)K, LLONG_MAX);
    HIPC(h, d_map.upload(a->map, (size_t)K, s));
    HIPC(h, d_ctr.fill(0, s));

    HIPC(h, timer.start(s));
    for (int m = 0; m < M; m++) {
        const int64_t n = h->N[m];
        if (n == 0) continue;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n / 4 + 255) / 256, (int64_t)h->num_cus * 8));
        LAUNCH(h, remap_z_kernel, dim3(grid), dim3(256), 0, s, mm.z[m], n, d_map.get(), K, d_ctr + 2 * m);
        h->st.assignments_replaced(m, h->st.view_unassigned(m) || f.drops[m]);
    }
    HIPC(h, dispatch_T(lt.T, [&](auto t) {
        hipLaunchKernelGGL(remap_fold_kernel<decltype(t)::value>, dim3(wave_blocks(nrows, h->num_cus)), dim3(256), lds, s, mm.counts, nrows, d_map.get(), K);
        return hipGetLastError();
    }));
    HIPC(h, timer.stop(s));
    if (h->st.delta16_used()) {                                // as mvhdp_build_counts: leftovers of a sweep that never reached its apply pass
        HIPC(h, hipMemsetD16Async(mm.delta16, (unsigned short)0x8000, (size_t)(mm.rowbase[M] * K), s));
        h->st.delta16_rebiased();
    }
    HIPC(h, hipMemcpyAsync(h->d_birth_table, none.data(), (size_t)K * sizeof(long long), hipMemcpyHostToDevice, s));
    u64 ctr[2 * MVHDP_MAXM] = {};
    HIPC(h, d_ctr.download(ctr, (size_t)2 * MVHDP_MAXM, s));
    HIPC(h, hipStreamSynchronize(s));
    HIPC(h, timer.elapsed_ms(&st.kernel_ms));

    h->h_alpha.swap(f.alpha);
    h->h_inactive.swap(f.inactive);
    mm.first_inactive = -1;
    for (int k = 0; k < K; k++) if (h->h_inactive[(size_t)k]) { mm.first_inactive = k; break; }
    HIPC(h, hipMemcpy(h->d_alpha, h->h_alpha.data(), h->h_alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMemcpy(h->d_inactive, h->h_inactive.data(), (size_t)K, hipMemcpyHostToDevice));
    h->st.counts_rebuilt();                                    // the counts are those of z again; the trees are not those of the counts
    for (int m = 0; m < M; m++) { st.moved[m] = (int64_t)ctr[2 * m]; st.dropped[m] = (int64_t)ctr[2 * m + 1]; }
    st.vacated = f.vacated; st.retired = f.retired;
    return MVHDP_OK;
}

} // namespace

// every refusal, in the header's order; nothing on the device or in the handle is touched
int mvhdp_remap_check(mvhdp_ctx* h, const mvhdp_remap_args* a)
{
    const int K = h->mm.K;
    if (!a || !a->map) FAIL(h, MVHDP_ERR_INVALID_ARG, "remap_topics: null args or map");
    if (a->flags & ~MVHDP_REMAP_RETIRE) FAIL(h, MVHDP_ERR_INVALID_ARG, "remap_topics: unknown flags");
    for (int k = 0; k < K; k++)
        if (a->map[k] < MVHDP_UNASSIGNED_TOPIC || a->map[k] >= K) FAIL(h, MVHDP_ERR_INVALID_ARG, "remap_topics: a map entry outside [-1, K)");
    if (int rc = require_corpus(h)) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "remap_topics before set_hyper");
    if (int rc = require_current_counts(h, "remap_topics")) return rc;
    if (h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "remap_topics inside an mvhdp_apply_delta_begin bracket (call mvhdp_apply_delta_end first)");
    if (h->mm.mix) FAIL(h, MVHDP_ERR_UNSUPPORTED, "remap_topics: a vectors mix is set, and its columns belong to topics (mvhdp_set_vectors_mix(h, 0, NULL, NULL) first)");
    if (mvhdp_emb_has_topic_rows(h)) FAIL(h, MVHDP_ERR_UNSUPPORTED, "remap_topics: embeddings with topic rows are initialised (mvhdp_emb_release first)");
    if (K > MVHDP_MAX_TOPICS) FAIL(h, MVHDP_ERR_UNSUPPORTED, "remap_topics: more than 2048 topics");
    return MVHDP_OK;
}

extern "C" int mvhdp_remap_topics(mvhdp_handle h, const mvhdp_remap_args* a, mvhdp_remap_stats* stats)
{
    CHECK_H(h);
    int rc = mvhdp_remap_check(h, a); if (rc) return rc;
    mvhdp_remap_stats st{};
    rc = remap_run(h, a, st); if (rc) return rc;
    if (stats) *stats = st;
    return MVHDP_OK;
}
