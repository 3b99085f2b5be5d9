// mvhdp_foldin.hip — fold-in of unseen documents on the trained handle: from the tokens of a batch of documents over the M views to their
// topic proportions, every Gibbs iteration inside one kernel, against the frozen counts where the handle keeps them (include/mvhdp.h has
// the contract: the dense conditional, the coupling, the counter, the samples; tests/native/foldin_ref.c restates it on the host).
//   foldin_kernel<T, VEC>   one wave per document for ALL iterations, pulled longest document first (tokens over the views) from one queue
//                           head.  Lane l owns the T topics l T .. l T + T - 1, as in heldout_ltr_kernel (the gather and the draw are
//                           mvhdp_lanes.h's).  The view in flight keeps its
//                           n_dk and base_m = a_m + o_m in registers (2 T values a lane), rinv_m too up to T = 8 (beyond that it is read
//                           from the call's table, which stays in L2); the other views' n_dk and the running counts_sum sit in a per-wave
//                           state slice [2][M][64 T] of int32, entry j * 64 + lane = topic lane * T + j: in LDS while the block's four
//                           slices fit FOLDIN_LDS_STATE_BYTES, else in a global scratch slice per resident wave.  A visit is the held-out
//                           kernel's: the count row of the NEXT position of the pass is requested before this visit's weights are formed,
//                           rows are read from the 32-bit table, and a document's rows come back `iterations` times and stay in L2.  z: the
//                           first FOLDIN_ZCAP positions of the document (its views' spans laid end to end) in LDS, 2 bytes each, the rest
//                           in the chunk's global z buffer, which also receives the LDS part when the document is done.  At the end the
//                           wave writes counts_sum and, if asked, theta with the expression of doc_topic_prop_kernel.
// Documents are cut into chunks on the host so that the per-chunk buffers (tokens 4 + z 2 bytes a token; counts_sum 4 M K and theta 8 K
// bytes a document) stay within FOLDIN_SCRATCH_BYTES (a chunk is at least one document); the global state slices, where used, are at most
// num_cus * 2 blocks x 4 waves x 2 M 64 T x 4 bytes (256 MiB at M = 8, K = 2048 on 256 CUs).  Everything runs on the handle's stream; the
// call only reads the handle (no ModelState transition).
#include "mvhdp_side.h"
#include "mvhdp_wave.h"
#include "mvhdp_lanes.h"

namespace {

constexpr int FOLDIN_ZCAP = 512;                               // positions of a document whose z stays in LDS (2 bytes each, per wave)
constexpr size_t FOLDIN_SCRATCH_BYTES = (size_t)256 << 20;     // per chunk: tokens, z, counts_sum, theta
constexpr size_t FOLDIN_LDS_STATE_BYTES = 48 * 1024;           // the four state slices of a block, beside the 4 KiB of z
constexpr int FOLDIN_NONE = 0xFFFF;                            // z of a token that holds no topic
typedef unsigned long long u64;

struct FoldinArgs {
    const int32_t* rows[MVHDP_MAXM];   // n_wk of view m: [V_m][K]
    const int64_t* doc_off[MVHDP_MAXM];// [Dc + 1] of the chunk, from 0; nullptr: no document has the view
    const int32_t* tok[MVHDP_MAXM];    // [Nc_m]
    uint16_t* zs[MVHDP_MAXM];          // [Nc_m] z of every position, FOLDIN_NONE at the start
    const double* tab;                 // [M][2][64 T]: a_m = gamma * alpha, then rinv_m (0 for an inactive topic); entry j * 64 + lane is topic lane * T + j (0 beyond K)
    const int32_t* order;              // [Dc] the chunk's documents by total length descending
    int32_t* state;                    // [blocks * 4][2][M][64 T], or nullptr: the slices are in LDS
    int32_t* counts_sum;               // [Dc][M][K]
    double* theta;                     // [Dc][K] or nullptr
    u64* head;
    int64_t n_docs, doc_global0;
    int32_t K, M, iterations, S, thin;
    int32_t V[MVHDP_MAXM];
    double beta[MVHDP_MAXM], gas[MVHDP_MAXM] /* gamma * alphaSum */, w[MVHDP_MAXM], P[MVHDP_MAXM * MVHDP_MAXM];
    uint32_t seed_lo, seed_hi;
};

template <int T, bool VEC>
__global__ __launch_bounds__(256) void foldin_kernel(const FoldinArgs a)
{
    extern __shared__ int32_t s_state[];                       // [4][2][M][64 T] unless a.state
    __shared__ uint16_t s_z[4][FOLDIN_ZCAP];
    constexpr int KT = 64 * T;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int K = a.K, M = a.M;
    int32_t* st = a.state ? a.state + ((int64_t)blockIdx.x * 4 + wv) * (2 * M * KT) : s_state + wv * (2 * M * KT);
    int32_t* nd = st;                                          // n_dk[m][..]
    int32_t* cs = st + M * KT;                                 // counts_sum[m][..]
    uint16_t* zl = s_z[wv];
    const int first_rec = a.iterations - (a.S - 1) * a.thin;

    for (;;) {                                                 // wave-uniform from here on; no barrier: the waves of a block go their own ways
        u64 qv = 0;
        if (lane == 0) qv = atomicAdd(a.head, 1ull);
        const int64_t q = uniform_i64((int64_t)qv);
        if (q >= a.n_docs) break;
        const int64_t dl = a.order[q];
        const u64 g = (u64)(a.doc_global0 + dl);
        const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);

        for (int i = lane; i < 2 * M * KT; i += 64) st[i] = 0;
        {
            int64_t total_len = 0;
            for (int m = 0; m < M; m++)
                if (a.doc_off[m]) total_len += a.doc_off[m][dl + 1] - a.doc_off[m][dl];
            const int nz = (int)(total_len < FOLDIN_ZCAP ? total_len : FOLDIN_ZCAP);
            for (int i = lane; i < nz; i += 64) zl[i] = (uint16_t)FOLDIN_NONE;
        }
        LDS_FENCE();

        for (int it = 1; it <= a.iterations; it++) {
            const bool rec = it >= first_rec && (a.iterations - it) % a.thin == 0;
            int64_t zc0 = 0;                                   // where view m's span starts in the document's z
            for (int m = 0; m < M; m++) {
                const int64_t* __restrict__ off = a.doc_off[m];
                if (!off) continue;
                const int64_t b = off[dl];
                const int L = (int)(off[dl + 1] - b);
                if (L <= 0) continue;
                const int32_t* __restrict__ tk = a.tok[m] + b;
                uint16_t* zg = a.zs[m] + b;                    // only positions at zc0 + pos >= FOLDIN_ZCAP are touched before the end
                const int32_t* __restrict__ rows = a.rows[m];
                const double* __restrict__ t_a = a.tab + (size_t)m * 2 * KT;
                const double* __restrict__ t_rinv = t_a + KT;
                const int V = a.V[m];
                const double beta = a.beta[m], pmm = a.P[m * MVHDP_MAXM + m];
                const double Lp_m = (double)L + a.gas[m];

                // ---- the pass's constants from the CURRENT counts of the other views ----
                int n[T];
                double base[T];
#pragma unroll
                for (int j = 0; j < T; j++) { n[j] = nd[m * KT + j * 64 + lane]; base[j] = 0.0; }
                for (int i = 0; i < M; i++) {
                    if (i == m || !a.doc_off[i]) continue;
                    const int len_i = (int)(a.doc_off[i][dl + 1] - a.doc_off[i][dl]);
                    if (len_i == 0) continue;
                    const double Lp_i = (double)len_i + a.gas[i], p = a.P[m * MVHDP_MAXM + i];
                    const double* __restrict__ a_i = a.tab + (size_t)i * 2 * KT;
#pragma unroll
                    for (int j = 0; j < T; j++) base[j] = base[j] + p * ((double)nd[i * KT + j * 64 + lane] + a_i[j * 64 + lane]) / Lp_i;
                }
#pragma unroll
                for (int j = 0; j < T; j++) base[j] = t_a[j * 64 + lane] + base[j] * Lp_m;
                double rinv[T <= 8 ? T : 1];
                if constexpr (T <= 8) {
#pragma unroll
                    for (int j = 0; j < T; j++) rinv[j] = t_rinv[j * 64 + lane];
                }

                // ---- the positions in order; the row of the next one is requested at the top of the turn ----
                int w = tk[0];
                int row[T], rown[T];
                if ((uint32_t)w < (uint32_t)V) gather_row<T, VEC>(rows, w, K, lane, row);
                else {
#pragma unroll
                    for (int j = 0; j < T; j++) row[j] = 0;
                }
                const uint32_t c2 = (uint32_t)it | ((uint32_t)m << 16);
                for (int pos = 0; pos < L; pos++) {
                    const int w_nxt = pos + 1 < L ? tk[pos + 1] : -1;
                    if ((uint32_t)w_nxt < (uint32_t)V) gather_row<T, VEC>(rows, w_nxt, K, lane, rown);
                    else {
#pragma unroll
                        for (int j = 0; j < T; j++) rown[j] = 0;
                    }

                    if ((uint32_t)w < (uint32_t)V) {           // an out-of-vocabulary token: never visited
                        const bool in_lds = zc0 + pos < FOLDIN_ZCAP;
                        int zo = 0;
                        if (lane == 0) zo = in_lds ? (int)zl[zc0 + pos] : (int)zg[pos];
                        zo = __builtin_amdgcn_readfirstlane(zo);
                        if (zo != FOLDIN_NONE) {               // take the token's topic out
                            const int mine = (zo / T == lane) ? (zo % T) : -1;
#pragma unroll
                            for (int j = 0; j < T; j++) n[j] -= (j == mine) ? 1 : 0;
                        }
                        double wt[T];
                        double s = 0.0;
#pragma unroll
                        for (int j = 0; j < T; j++) {
                            double ri;
                            if constexpr (T <= 8) ri = rinv[j]; else ri = t_rinv[j * 64 + lane];
                            const double phi = ((double)row[j] + beta) * ri;
                            wt[j] = (pmm * (double)n[j] + base[j]) * phi;
                            s = j == 0 ? wt[0] : s + wt[j];
                        }
                        const double incl = wave_incl_scan_d_dpp(s);
                        const double total = bcast_d(incl, 63);
                        double excl = __shfl_up(incl, 1, 64);
                        if (lane == 0) excl = 0.0;
                        uint32_t x[4];
                        philox4x32_10(c0, c1, c2, (uint32_t)pos, a.seed_lo, a.seed_hi, x);
                        const double target = bits_to_unit(x[0], x[1]) * total;
                        int sel_lane, sel_j;
                        lane_draw<T>(wt, excl, target, sel_lane, sel_j);
                        const bool drawn = total > 0.0 && total <= 1.7976931348623157e308;   // 0.0 or not finite: the token stays as it was
                        const int zn = drawn ? sel_lane * T + sel_j : zo;
                        if (zn != FOLDIN_NONE) {
                            const int mine = (zn / T == lane) ? (zn % T) : -1;
#pragma unroll
                            for (int j = 0; j < T; j++) n[j] += (j == mine) ? 1 : 0;
                        }
                        if (lane == 0 && drawn) {
                            if (in_lds) zl[zc0 + pos] = (uint16_t)zn; else zg[pos] = (uint16_t)zn;
                        }
                    }
                    w = w_nxt;
#pragma unroll
                    for (int j = 0; j < T; j++) row[j] = rown[j];
                }

#pragma unroll
                for (int j = 0; j < T; j++) {
                    nd[m * KT + j * 64 + lane] = n[j];
                    if (rec) cs[m * KT + j * 64 + lane] += n[j];
                }
                zc0 += L;
            }
        }

        // ---- the document's outputs ----
        LDS_FENCE();
        {
            int64_t zc0 = 0;
            for (int m = 0; m < M; m++) {
                if (!a.doc_off[m]) continue;
                const int64_t b = a.doc_off[m][dl], L = a.doc_off[m][dl + 1] - b;
                for (int64_t i = lane; i < L && zc0 + i < FOLDIN_ZCAP; i += 64) a.zs[m][b + i] = zl[zc0 + i];
                zc0 += L;
            }
        }
        for (int m = 0; m < M; m++) {
            int32_t* __restrict__ o = a.counts_sum + (dl * M + m) * K;
#pragma unroll
            for (int j = 0; j < T; j++) {
                const int k = lane * T + j;
                if (k < K) o[k] = cs[m * KT + j * 64 + lane];
            }
        }
        if (a.theta) {                                         // the expression of doc_topic_prop_kernel, n_dk replaced by counts_sum / S
            double norm = 0;
            for (int m = 0; m < M; m++) norm += a.w[m];
            double* __restrict__ o = a.theta + dl * K;
            const double Sd = (double)a.S;
#pragma unroll
            for (int j = 0; j < T; j++) {
                const int k = lane * T + j;
                if (k >= K) continue;
                double tp = 0;
                for (int m = 0; m < M; m++) {
                    const int len = a.doc_off[m] ? (int)(a.doc_off[m][dl + 1] - a.doc_off[m][dl]) : 0;
                    tp += a.w[m] * ((double)cs[m * KT + j * 64 + lane] / Sd + a.tab[(size_t)m * 2 * KT + j * 64 + lane]) / (len + a.gas[m]);
                }
                o[k] = tp / norm;
            }
        }
        LDS_FENCE();
    }
}

template <int T>
hipError_t launch_foldin(const FoldinArgs& ka, bool vec, unsigned blocks, size_t lds, hipStream_t s)
{
    if constexpr (T >= 4) {
        if (vec) { hipLaunchKernelGGL((foldin_kernel<T, true>), dim3(blocks), dim3(256), lds, s, ka); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((foldin_kernel<T, false>), dim3(blocks), dim3(256), lds, s, ka);
    return hipGetLastError();
}

} // namespace

extern "C" int mvhdp_fold_in(mvhdp_handle h, const mvhdp_foldin_args* a, int64_t num_docs, const int64_t* const* doc_off, const int32_t* const* tokens,
                             double* theta, int32_t* const* z, int32_t* counts_sum, mvhdp_foldin_stats* stats)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K, M = mm.M;
    if (!a || num_docs < 0 || !doc_off || !tokens) FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: null argument or negative num_docs");
    if (a->iterations < 1 || a->iterations > 65535) FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: iterations outside 1..65535");
    if (a->samples < 1 || a->thin < 1 || (int64_t)a->iterations - ((int64_t)a->samples - 1) * a->thin < 1)
        FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: samples and thin must be >= 1 and every recorded iteration >= 1");
    if (a->doc_base < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: negative doc_base");
    const std::string who("fold_in: ");
    if (a->coupling)
        if (const char* r = check_nonneg_finite(a->coupling, (int64_t)M * M)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + "a coupling entry " + r);
    if (theta) {
        if (!a->view_weights) FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: theta without view_weights");
        if (const char* r = check_view_weights(a->view_weights, M)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + r);
    }
    int64_t N[MVHDP_MAXM] = {};
    for (int m = 0; m < M; m++) {
        const int64_t* off = doc_off[m];
        if (!off) continue;
        if (const char* r = check_offsets(off, num_docs, INT32_MAX)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + "doc_off (a span: at most 2^31 - 1 tokens) " + r);
        N[m] = off[num_docs];
        if (N[m] > 0 && !tokens[m]) FAIL(h, MVHDP_ERR_INVALID_ARG, "fold_in: null tokens");
        if (const char* r = check_tokens_nonneg(tokens[m], N[m])) FAIL(h, MVHDP_ERR_INVALID_ARG, who + r);
    }
    if (K > 64 * 32) FAIL(h, MVHDP_ERR_UNSUPPORTED, "fold_in: more than 2048 topics");   // (mvhdp_create admits none: MVHDP_MAX_TOPICS)
    // the counts as the handle holds them: stale counts, or counts that lack a NO_APPLY sweep's pending deltas, are taken as they are (the header says so)
    if (!h->have_hyper || !h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "fold_in before set_hyper / counts (build_counts, set_counts or a sweep)");
    mvhdp_foldin_stats st{};
    if (num_docs == 0) { if (stats) *stats = st; return MVHDP_OK; }
    if (int rc = side_begin(h)) return rc;

    // ---- the frozen model in the order the lanes read it ----
    const LaneTiling lt = lane_tiling(K);
    const int T = lt.T, KT = 64 * T;
    const bool vec = lt.vec;
    std::vector<int32_t> nk((size_t)M * K);
    HIPC(h, hipMemcpyAsync(nk.data(), mm.counts + mm.rowbase[M] * K, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::vector<double> tab((size_t)M * 2 * KT, 0.0);
    for (int m = 0; m < M; m++)
        for (int k = 0; k < K; k++) {
            const size_t at = (size_t)m * 2 * KT + lane_slot(k, T);
            tab[at] = mm.gamma[m] * h->h_alpha[(size_t)m * (K + 1) + k];
            const bool off_topic = !h->h_inactive.empty() && h->h_inactive[(size_t)k] != 0;
            tab[at + KT] = off_topic ? 0.0 : 1.0 / ((double)nk[(size_t)m * K + k] + mm.beta_sum[m]);   // phi of an inactive topic is exactly 0.0
        }
    FoldinArgs ka{};
    for (int m = 0; m < M; m++) {
        ka.rows[m] = mm.counts + mm.rowbase[m] * K;
        ka.V[m] = mm.V[m];
        ka.beta[m] = mm.beta[m];
        ka.gas[m] = mm.gamma[m] * mm.alpha_sum[m];
        ka.w[m] = theta ? a->view_weights[m] : 0.0;
        for (int i = 0; i < M; i++) {
            double p;
            if (a->coupling) p = a->coupling[m * M + i];
            else if (i == m) p = 1.0;
            else p = mm.p_a[m][i] == 0.0 ? 0.0 : mm.p_a[m][i] / (mm.p_a[m][i] + mm.p_b[m][i]);
            ka.P[m * MVHDP_MAXM + i] = p;
        }
    }
    ka.K = K; ka.M = M; ka.iterations = a->iterations; ka.S = a->samples; ka.thin = a->thin;
    ka.seed_lo = (uint32_t)a->seed; ka.seed_hi = (uint32_t)(a->seed >> 32);
    DevArray<double> d_tab;
    DevArray<u64> d_head;
    DevArray<int32_t> d_state;
    HIPC(h, d_tab.alloc(tab.size()));
    HIPC(h, d_head.alloc(1));
    HIPC(h, d_tab.upload(tab.data(), tab.size(), h->stream));
    ka.tab = d_tab; ka.head = d_head;
    const size_t slice_ints = (size_t)2 * M * KT;
    const bool lds_state = 4 * slice_ints * sizeof(int32_t) <= FOLDIN_LDS_STATE_BYTES;
    const int64_t max_blocks = (int64_t)h->num_cus * (lds_state ? 8 : 2);
    StreamTimer timer;                                         // the kernel's time on the stream, chunk by chunk
    HIPC(h, timer.create());

    // ---- what the host can count ----
    std::vector<int64_t> doc_len((size_t)num_docs, 0);
    for (int m = 0; m < M; m++) {
        if (!doc_off[m]) continue;
        for (int64_t d = 0; d < num_docs; d++) doc_len[(size_t)d] += doc_off[m][d + 1] - doc_off[m][d];
        int64_t c = 0;
        for (int64_t i = 0; i < N[m]; i++) c += tokens[m][i] < mm.V[m];
        st.tokens += c;
        st.oov += N[m] - c;
    }
    st.visits = st.tokens * a->iterations;

    // ---- chunk by chunk ----
    const bool want_z = z != nullptr;
    std::vector<double> h_theta(theta ? (size_t)num_docs * K : 0);
    std::vector<int32_t> h_cs(counts_sum ? (size_t)num_docs * M * K : 0);
    std::vector<uint16_t> h_z[MVHDP_MAXM];
    if (want_z)
        for (int m = 0; m < M; m++)
            if (z[m] && doc_off[m]) h_z[m].resize((size_t)N[m]);
    const size_t doc_bytes = (size_t)K * (8 + 4 * (size_t)M);
    std::vector<int64_t> c_off;
    std::vector<int32_t> c_order;
    double kernel_ms = 0.0;
    for (int64_t d0 = 0; d0 < num_docs;) {
        int64_t d1 = d0;
        size_t bytes = 0;
        do { bytes += doc_bytes + (size_t)doc_len[(size_t)d1] * 6; d1++; }
        while (d1 < num_docs && bytes + doc_bytes + (size_t)doc_len[(size_t)d1] * 6 <= FOLDIN_SCRATCH_BYTES && d1 - d0 < (int64_t)INT32_MAX);
        const int64_t Dc = d1 - d0;
        order_by_length_desc(c_order, Dc, [&](int32_t d) { return doc_len[(size_t)(d0 + d)]; });
        DevArray<int64_t> d_off[MVHDP_MAXM];
        DevArray<int32_t> d_tok[MVHDP_MAXM], d_order, d_cs;
        DevArray<uint16_t> d_zs[MVHDP_MAXM];
        DevArray<double> d_theta;
        c_off.resize((size_t)Dc + 1);
        for (int m = 0; m < M; m++) {
            ka.doc_off[m] = nullptr; ka.tok[m] = nullptr; ka.zs[m] = nullptr;
            if (!doc_off[m]) continue;
            const int64_t t0 = doc_off[m][d0], Nc = doc_off[m][d1] - t0;
            for (int64_t d = 0; d <= Dc; d++) c_off[(size_t)d] = doc_off[m][d0 + d] - t0;
            HIPC(h, d_off[m].alloc((size_t)Dc + 1));
            HIPC(h, d_tok[m].alloc((size_t)Nc));
            HIPC(h, d_zs[m].alloc((size_t)Nc));
            HIPC(h, d_off[m].upload(c_off.data(), (size_t)Dc + 1, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));          // c_off is reused for the next view
            if (Nc > 0) HIPC(h, d_tok[m].upload(tokens[m] + t0, (size_t)Nc, h->stream));
            HIPC(h, d_zs[m].fill(0xFF, h->stream));
            ka.doc_off[m] = d_off[m]; ka.tok[m] = d_tok[m]; ka.zs[m] = d_zs[m];
        }
        HIPC(h, d_order.alloc((size_t)Dc));
        HIPC(h, d_cs.alloc((size_t)Dc * M * K));
        if (theta) HIPC(h, d_theta.alloc((size_t)Dc * K));
        HIPC(h, d_order.upload(c_order.data(), (size_t)Dc, h->stream));
        HIPC(h, d_head.fill(0, h->stream));
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((Dc + 7) / 8, max_blocks));
        if (!lds_state && d_state.size() < (size_t)blocks * 4 * slice_ints) HIPC(h, d_state.alloc((size_t)blocks * 4 * slice_ints));
        ka.order = d_order; ka.counts_sum = d_cs; ka.theta = theta ? d_theta.get() : nullptr;
        ka.state = lds_state ? nullptr : d_state.get();
        ka.n_docs = Dc; ka.doc_global0 = a->doc_base + d0;
        const size_t lds = lds_state ? 4 * slice_ints * sizeof(int32_t) : 0;
        HIPC(h, timer.start(h->stream));
        const hipError_t e = dispatch_T(T, [&](auto t) { return launch_foldin<decltype(t)::value>(ka, vec, blocks, lds, h->stream); });
        HIPC(h, e);
        HIPC(h, timer.stop(h->stream));
        if (theta) HIPC(h, d_theta.download(h_theta.data() + (size_t)d0 * K, (size_t)Dc * K, h->stream));
        if (counts_sum) HIPC(h, d_cs.download(h_cs.data() + (size_t)d0 * M * K, (size_t)Dc * M * K, h->stream));
        for (int m = 0; m < M; m++)
            if (!h_z[m].empty()) {
                const int64_t t0 = doc_off[m][d0], Nc = doc_off[m][d1] - t0;
                if (Nc > 0) HIPC(h, d_zs[m].download(h_z[m].data() + t0, (size_t)Nc, h->stream));
            }
        HIPC(h, hipStreamSynchronize(h->stream));
        double ms = 0.0;
        HIPC(h, timer.elapsed_ms(&ms));
        kernel_ms += ms;
        d0 = d1;
    }

    st.kernel_ms = kernel_ms;
    if (theta) memcpy(theta, h_theta.data(), h_theta.size() * sizeof(double));
    if (counts_sum) memcpy(counts_sum, h_cs.data(), h_cs.size() * sizeof(int32_t));
    for (int m = 0; m < M; m++)
        for (size_t i = 0; i < h_z[m].size(); i++) z[m][i] = h_z[m][i] == FOLDIN_NONE ? -1 : (int32_t)h_z[m][i];
    if (stats) *stats = st;
    return MVHDP_OK;
}
