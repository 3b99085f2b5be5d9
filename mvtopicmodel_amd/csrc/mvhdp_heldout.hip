// mvhdp_heldout.hip — held-out evaluation: the left-to-right document likelihood of Wallach et al. 2009 as MALLET's
// MarginalProbEstimator.evaluateLeftToRight runs it, with the arguments of getMALLETProbEstimator (PTM:3470-3478), against the frozen
// counts of one view (include/mvhdp.h has the contract, the summation order included; tests/native/ltr_ref.c restates it on the host).
//   heldout_ltr_kernel<T, VEC>   one wave per (document, particle), pulled longest document first from one queue head.  Lane l owns the T
//                                topics l T .. l T + T - 1 (T = 1, 2, 4, .. 32, the smallest with 64 T >= K): their n_dk sit in its
//                                registers, their alpha and 1 / (n_k + betaSum) in LDS ([j][lane], one conflict-free read per j), staged once
//                                per block.  A visit gathers the token's count row (lane l its T cells; VEC: K a multiple of 4, 16-byte loads),
//                                forms the T weights with two multiplies each, sums them in the lane, scans the 64 lane sums
//                                (wave_incl_scan_d_dpp), and draws: every lane searches its own topics against u * total, a ballot names the
//                                first lane that found one.  The row of the NEXT visit is requested before the weights of this one are
//                                formed (its token was read a visit earlier), so the gather waits behind arithmetic, not in front of it.  The
//                                rows are read where they are: a document's rows come back L - j times and stay in L2.  z: LDS for the
//                                first HELDOUT_ZCAP positions of the document, a global scratch beyond.  resample = 0: the inner positions
//                                are never visited.  No divide but the one that scores a position.
//   heldout_reduce_kernel        one wave per document: S[n] = the particles' p_r[n] added in ascending r, and the document's sum of
//                                log S[n] - log R in a fixed order.
// Work is cut into document chunks on the host so that the per-particle buffers (p_r[n]: 8 bytes, z beyond the cap: 2 bytes, per particle and
// token) stay within HELDOUT_SCRATCH_BYTES.  Everything runs on the handle's stream.
#include "mvhdp_side.h"
#include "mvhdp_wave.h"
#include "mvhdp_lanes.h"

namespace {

constexpr int HELDOUT_ZCAP = 512;                              // positions of a document whose z stays in LDS (2 bytes each, per wave)
constexpr size_t HELDOUT_SCRATCH_BYTES = (size_t)256 << 20;    // per chunk: particles x tokens x 10 bytes at most (a chunk is at least one document)
constexpr int HELDOUT_MAX_PARTICLES = 1 << 20;                 // the particle shares a Philox counter word with the high bits of the document id
typedef unsigned long long u64;

struct HeldoutArgs {
    const int32_t* rows;               // n_wk of the view: [V][K]
    const double* tab;                 // [2][64 T]: alpha, then 1 / (n_k + betaSum); entry j * 64 + lane is topic lane * T + j (0 beyond K)
    const int64_t* doc_off;            // [Dc + 1] of the chunk, from 0
    const int32_t* tok;                // [Nc]
    const int32_t* order;              // [Dc] the chunk's documents by length descending
    uint16_t* zs;                      // [R][Nc] z of the positions beyond HELDOUT_ZCAP, or nullptr: no document is that long
    double* P;                         // [R][Nc] p_r[n]; written for every in-vocabulary position
    u64* head;                         // the queue: item q = (document order[q / R], particle q % R)
    int64_t n_items, Nc, doc_global0;  // doc_global0: the global index of the chunk's first document
    int32_t K, V, R, resample;
    double beta, alpha_sum;
    uint32_t seed_lo, seed_hi;
};

template <int T, bool VEC>
__global__ __launch_bounds__(256) void heldout_ltr_kernel(const HeldoutArgs a)
{
    __shared__ double s_tab[2 * 64 * T];
    __shared__ uint16_t s_z[4][HELDOUT_ZCAP];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 2 * 64 * T; i += 256) s_tab[i] = a.tab[i];
    __syncthreads();
    const double* __restrict__ s_alpha = s_tab;
    const double* __restrict__ s_rinv = s_tab + 64 * T;
    uint16_t* zl = s_z[threadIdx.x >> 6];
    const int K = a.K, V = a.V, R = a.R;
    const bool resample = a.resample != 0;
    const double beta = a.beta;

    for (;;) {                                                 // wave-uniform from here on; no barrier: the waves of a block go their own ways
        u64 qv = 0;
        if (lane == 0) qv = atomicAdd(a.head, 1ull);
        const int64_t q = uniform_i64((int64_t)qv);
        if (q >= a.n_items) break;
        const int64_t dl = a.order[q / R];
        const int r = (int)(q % R);
        const int64_t b = a.doc_off[dl];
        const int L = (int)(a.doc_off[dl + 1] - b);
        if (L <= 0) continue;
        const int32_t* __restrict__ tk = a.tok + b;
        double* __restrict__ Pr = a.P + (int64_t)r * a.Nc + b;
        uint16_t* zg = a.zs ? a.zs + (int64_t)r * a.Nc + b : nullptr;     // only positions >= HELDOUT_ZCAP are touched
        const u64 g = (u64)(a.doc_global0 + dl);
        const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)r + ((uint32_t)(g >> 32) << 20);

        int n[T];
#pragma unroll
        for (int j = 0; j < T; j++) n[j] = 0;
        int tokens_so_far = 0;

        // The visits in order: (limit, pos), pos = 0 .. limit - 1 (resample only), then pos = limit, which scores.  `cur` is the visit of this
        // turn, `nxt` the one after it (its token is known, its row is requested at the top of the turn), `nn` the one after that (its token is read).
        int limit = 0, pos = 0;
        int w = tk[0];
        int n_limit = pos < limit ? limit : limit + 1, n_pos = pos < limit ? pos + 1 : (resample ? 0 : limit + 1);
        int w_nxt = n_limit < L ? tk[n_pos] : -1;
        int row[T], rown[T];
        if ((uint32_t)w < (uint32_t)V) gather_row<T, VEC>(a.rows, w, K, lane, row);
        else {
#pragma unroll
            for (int j = 0; j < T; j++) row[j] = 0;
        }
        while (limit < L) {
            const int nn_limit = n_pos < n_limit ? n_limit : n_limit + 1, nn_pos = n_pos < n_limit ? n_pos + 1 : (resample ? 0 : n_limit + 1);
            int w_nn = -1;
            if (n_limit < L && nn_limit < L) w_nn = tk[nn_pos];
            const bool nxt_valid = n_limit < L && (uint32_t)w_nxt < (uint32_t)V;
            if (nxt_valid) gather_row<T, VEC>(a.rows, w_nxt, K, lane, rown);
            else {
#pragma unroll
                for (int j = 0; j < T; j++) rown[j] = 0;
            }

            if ((uint32_t)w < (uint32_t)V) {                   // an out-of-vocabulary token: nothing happens
                const bool score = pos == limit;
                if (!score) {                                  // take z[pos] out
                    int zo = 0;
                    if (lane == 0) zo = pos < HELDOUT_ZCAP ? (int)zl[pos] : (int)zg[pos];
                    zo = __builtin_amdgcn_readfirstlane(zo);
                    const int mine = (zo / T == lane) ? (zo % T) : -1;
#pragma unroll
                    for (int j = 0; j < T; j++) n[j] -= (j == mine) ? 1 : 0;
                }
                double wt[T];
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < T; j++) {
                    const double phi = ((double)row[j] + beta) * s_rinv[j * 64 + lane];
                    wt[j] = (s_alpha[j * 64 + lane] + (double)n[j]) * phi;
                    s = j == 0 ? wt[0] : s + wt[j];
                }
                const double incl = wave_incl_scan_d_dpp(s);
                const double total = bcast_d(incl, 63);
                double excl = __shfl_up(incl, 1, 64);
                if (lane == 0) excl = 0.0;
                if (score) {
                    const double p = total / (a.alpha_sum + (double)tokens_so_far);
                    if (lane == 0) Pr[limit] = p;
                    tokens_so_far++;
                }
                uint32_t x[4];
                philox4x32_10(c0, c1, (uint32_t)limit, (uint32_t)pos, a.seed_lo, a.seed_hi, x);
                const double target = bits_to_unit(x[0], x[1]) * total;
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
                int sel_lane = 0, sel_j = 0;
                const u64 found = __builtin_amdgcn_ballot_w64(cand >= 0);
                if (found) {
                    sel_lane = __builtin_ctzll(found);
                    sel_j = bcast_i(cand, sel_lane);
                } else {
                    const u64 any = __builtin_amdgcn_ballot_w64(last >= 0);
                    if (any) {
                        sel_lane = 63 - __builtin_clzll(any);
                        sel_j = bcast_i(last, sel_lane);
                    }
                }
                const int mine = lane == sel_lane ? sel_j : -1;
#pragma unroll
                for (int j = 0; j < T; j++) n[j] += (j == mine) ? 1 : 0;
                if (lane == 0) {
                    const uint16_t zv = (uint16_t)(sel_lane * T + sel_j);
                    if (pos < HELDOUT_ZCAP) zl[pos] = zv; else zg[pos] = zv;
                }
            }
            limit = n_limit; pos = n_pos; w = w_nxt;
            n_limit = nn_limit; n_pos = nn_pos; w_nxt = w_nn;
#pragma unroll
            for (int j = 0; j < T; j++) row[j] = rown[j];
        }
    }
}

// one wave per document: S[n] and the document's log-likelihood.  Lane l adds its positions l, l + 64, .. in ascending order, the 64 lane sums
// are combined by the butterfly 32, 16, .. 1.
__global__ __launch_bounds__(256) void heldout_reduce_kernel(const double* __restrict__ P, const int64_t* __restrict__ doc_off, const int32_t* __restrict__ tok,
                                                             int64_t Dc, int64_t Nc, int V, int R, double log_r, double* __restrict__ S, double* __restrict__ doc_ll)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t d = wave; d < Dc; d += nwaves) {
        const int64_t b = doc_off[d], e = doc_off[d + 1];
        double acc = 0.0;
        for (int64_t i = b + lane; i < e; i += 64) {
            double s = 0.0;
            if ((uint32_t)tok[i] < (uint32_t)V)
                for (int r = 0; r < R; r++) s = s + P[(int64_t)r * Nc + i];
            S[i] = s;
            if (s > 0.0) acc = acc + (log(s) - log_r);
        }
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
        if (lane == 0) doc_ll[d] = acc;
    }
}


template <int T>
hipError_t launch_ltr(const HeldoutArgs& ka, bool vec, unsigned blocks, hipStream_t s)
{
    if constexpr (T >= 4) {
        if (vec) { hipLaunchKernelGGL((heldout_ltr_kernel<T, true>), dim3(blocks), dim3(256), 0, s, ka); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((heldout_ltr_kernel<T, false>), dim3(blocks), dim3(256), 0, s, ka);
    return hipGetLastError();
}

} // namespace

extern "C" int mvhdp_heldout_left_to_right(mvhdp_handle h, const mvhdp_heldout_args* a, int64_t num_docs, const int64_t* doc_off, const int32_t* tokens,
                                           double* doc_ll, double* position_sum, int64_t* doc_tokens, mvhdp_heldout_stats* stats)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (!a || num_docs < 0 || !doc_off) FAIL(h, MVHDP_ERR_INVALID_ARG, "heldout_left_to_right: null argument or negative num_docs");
    if (a->m < 0 || a->m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "heldout_left_to_right: bad view");
    if (a->particles < 1 || a->particles > HELDOUT_MAX_PARTICLES) FAIL(h, MVHDP_ERR_INVALID_ARG, "heldout_left_to_right: particles outside 1..2^20");
    if (a->doc_base < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "heldout_left_to_right: negative doc_base");
    const std::string who("heldout_left_to_right: ");
    if (const char* r = check_offsets(doc_off, num_docs, INT32_MAX)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + "doc_off (a span: at most 2^31 - 1 tokens) " + r);
    const int64_t N = doc_off[num_docs];
    if (N > 0 && !tokens) FAIL(h, MVHDP_ERR_INVALID_ARG, "heldout_left_to_right: null tokens");
    if (const char* r = check_tokens_nonneg(tokens, N)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + r);
    if (K > 64 * 32) FAIL(h, MVHDP_ERR_UNSUPPORTED, "heldout_left_to_right: more than 2048 topics");   // (mvhdp_create admits none: MVHDP_MAX_TOPICS)
    // the counts as the handle holds them: stale counts, or counts that lack a NO_APPLY sweep's pending deltas, are evaluated as they are (the header says so)
    if (!h->have_hyper || !h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "heldout_left_to_right before set_hyper / counts (build_counts, set_counts or a sweep)");
    const int m = a->m, V = mm.V[m], R = a->particles;
    const bool resample = a->resample != 0;
    if (int rc = side_begin(h)) return rc;

    // ---- the frozen model: alpha, 1 / (n_k + betaSum), in the order the lanes read them ----
    const LaneTiling lt = lane_tiling(K);
    const int T = lt.T;
    const bool vec = lt.vec;
    std::vector<int32_t> nk((size_t)K);
    HIPC(h, hipMemcpyAsync(nk.data(), mm.counts + mm.rowbase[mm.M] * K + (int64_t)m * K, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const double beta = mm.beta[m], beta_sum = beta * (double)V;                       // as MarginalProbEstimator's constructor: beta * numTypes
    const double* alpha = a->alpha ? a->alpha : h->h_alpha.data() + (size_t)m * (K + 1);   // alpha[m][k] unscaled beside gamma * alphaSum: PTM:3476
    const double alpha_sum = a->alpha ? a->alpha_sum : mm.gamma[m] * mm.alpha_sum[m];
    std::vector<double> tab((size_t)2 * 64 * T, 0.0);
    for (int k = 0; k < K; k++) {
        const size_t at = lane_slot(k, T);
        tab[at] = alpha[k];
        tab[(size_t)64 * T + at] = 1.0 / ((double)nk[(size_t)k] + beta_sum);
    }
    DevArray<double> d_tab;
    DevArray<u64> d_head;
    HIPC(h, d_tab.alloc(tab.size()));
    HIPC(h, d_head.alloc(1));
    HIPC(h, d_tab.upload(tab.data(), tab.size(), h->stream));

    // ---- what the host can count ----
    mvhdp_heldout_stats st{};
    std::vector<int64_t> h_doc_tokens((size_t)num_docs, 0);
    for (int64_t d = 0; d < num_docs; d++) {
        int64_t c = 0, vis = 0;
        for (int64_t i = doc_off[d]; i < doc_off[d + 1]; i++) {
            if (resample) vis += c;
            if (tokens[i] < V) { c++; vis++; }
        }
        h_doc_tokens[(size_t)d] = c;
        st.tokens += c;
        st.oov += doc_off[d + 1] - doc_off[d] - c;
        st.visits += vis * R;
    }

    // ---- chunk by chunk ----
    std::vector<double> h_S((size_t)N, 0.0), h_ll((size_t)num_docs, 0.0);
    const int64_t chunk_tokens = std::max<int64_t>(1, (int64_t)(HELDOUT_SCRATCH_BYTES / ((size_t)R * 10)));
    std::vector<int64_t> c_off;
    std::vector<int32_t> c_order;
    for (int64_t d0 = 0; d0 < num_docs;) {
        int64_t d1 = d0 + 1;
        while (d1 < num_docs && doc_off[d1 + 1] - doc_off[d0] <= chunk_tokens && d1 - d0 < (int64_t)INT32_MAX) d1++;
        const int64_t Dc = d1 - d0, t0 = doc_off[d0], Nc = doc_off[d1] - t0;
        if (Nc > 0) {
            c_off.resize((size_t)Dc + 1);
            int64_t longest = 0;
            for (int64_t d = 0; d <= Dc; d++) c_off[(size_t)d] = doc_off[d0 + d] - t0;
            for (int64_t d = 0; d < Dc; d++) longest = std::max(longest, c_off[(size_t)d + 1] - c_off[(size_t)d]);
            order_by_length_desc(c_order, Dc, [&](int32_t d) { return c_off[(size_t)d + 1] - c_off[(size_t)d]; });
            DevArray<int64_t> d_off;
            DevArray<int32_t> d_tok, d_order;
            DevArray<uint16_t> d_zs;
            DevArray<double> d_P, d_S, d_ll;
            HIPC(h, d_off.alloc((size_t)Dc + 1));
            HIPC(h, d_tok.alloc((size_t)Nc));
            HIPC(h, d_order.alloc((size_t)Dc));
            HIPC(h, d_P.alloc((size_t)R * Nc));
            HIPC(h, d_S.alloc((size_t)Nc));
            HIPC(h, d_ll.alloc((size_t)Dc));
            if (longest > HELDOUT_ZCAP) HIPC(h, d_zs.alloc((size_t)R * Nc));
            HIPC(h, d_off.upload(c_off.data(), (size_t)Dc + 1, h->stream));
            HIPC(h, d_tok.upload(tokens + t0, (size_t)Nc, h->stream));
            HIPC(h, d_order.upload(c_order.data(), (size_t)Dc, h->stream));
            HIPC(h, d_head.fill(0, h->stream));
            HeldoutArgs ka{};
            ka.rows = mm.counts + mm.rowbase[m] * K;
            ka.tab = d_tab;
            ka.doc_off = d_off; ka.tok = d_tok; ka.order = d_order;
            ka.zs = d_zs; ka.P = d_P; ka.head = d_head;
            ka.n_items = Dc * R; ka.Nc = Nc; ka.doc_global0 = a->doc_base + d0;
            ka.K = K; ka.V = V; ka.R = R; ka.resample = resample ? 1 : 0;
            ka.beta = beta; ka.alpha_sum = alpha_sum;
            ka.seed_lo = (uint32_t)a->seed; ka.seed_hi = (uint32_t)(a->seed >> 32);
            const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ka.n_items + 7) / 8, (int64_t)h->num_cus * 8));   // two items a wave at least: the tables are staged once per block
            const hipError_t e = dispatch_T(T, [&](auto t) { return launch_ltr<decltype(t)::value>(ka, vec, blocks, h->stream); });
            HIPC(h, e);
            const unsigned rblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((Dc + 3) / 4, (int64_t)h->num_cus * 8));
            LAUNCH(h, heldout_reduce_kernel, dim3(rblocks), dim3(256), 0, h->stream, d_P, d_off, d_tok, Dc, Nc, V, R, std::log((double)R), d_S, d_ll);
            HIPC(h, d_S.download(h_S.data() + t0, (size_t)Nc, h->stream));
            HIPC(h, d_ll.download(h_ll.data() + d0, (size_t)Dc, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
        }
        d0 = d1;
    }
    HIPC(h, hipStreamSynchronize(h->stream));

    double total = 0.0;
    for (int64_t d = 0; d < num_docs; d++) total = total + h_ll[(size_t)d];
    st.log_likelihood = total;
    if (doc_ll && num_docs) memcpy(doc_ll, h_ll.data(), (size_t)num_docs * sizeof(double));
    if (position_sum && N) memcpy(position_sum, h_S.data(), (size_t)N * sizeof(double));
    if (doc_tokens && num_docs) memcpy(doc_tokens, h_doc_tokens.data(), (size_t)num_docs * sizeof(int64_t));
    if (stats) *stats = st;
    return MVHDP_OK;
}
