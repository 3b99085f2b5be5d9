// mvhdp_nearest.hip — retrieval on a trained model (include/mvhdp.h has the contracts, mvhdp_nearest.h the geometry and the argument why
// the screen never decides; tests/nearest_numpy.py restates both entry points):
//   mvhdp_nearest_entities     per query row the n candidate entities of largest cosine, by the fp64 chain of mvhdp_similar_pairs
//   mvhdp_topic_top_entities   per topic the n entities of largest proportion
// The proportions are produced on the device (mvhdp_launch_doc_topic_prop) and stay there.
// Both sets of rows are prepared as mvhdp_similar_pairs prepares its own (mvhdp_screen_prepare_rows: cleaned, norms, classes, fp32 image).
//   near_screen_kernel         the screen: 128 queries x 128 candidates per block on v_mfma_f32_32x32x2_f32; every cell is written to the
//                              block of scores [queries of the block][candidates of the stripe] as an order-preserving 32-bit key, 0 for a
//                              cell that is not screened (a row that is not tame, padding, the query itself)
//   near_select_kernel         one wave per query: the stripe's keys in LDS, the n-th largest key over them and the n largest of the
//                              stripes before (a bitwise descent, as wave_first_n does on 64-bit keys, on the few keys that reach
//                              the n-th largest of the lanes' maxima where that bound exists), the n largest kept for the next stripe, and the cells that pass appended with ONE atomic per query and stripe
//   near_group_kernel          the block's candidates placed query by query (integer atomics: the order inside a query is not kept, and
//                              nothing depends on it)
//   near_exact_kernel          every candidate recomputed by the fp64 chain
//   near_pick_kernel           one wave per query: the first n by (sim descending, id ascending): wave_first_n (mvhdp_select.h) on the
//                              composite (key of the fp64 bits, ~id)
//   topk_partial_kernel        a thread per (slice of entities, topic), lanes over topics: the n largest proportions of the slice
//   topk_merge_kernel          one wave per topic: the first n of all slices, by wave_first_n as well
// No floating-point atomics: every fp64 value is a chain in a fixed order, integers and exact fp64 values decide every comparison.
#include "mvhdp_screen.h"
#include "mvhdp_select.h"
#include "mvhdp_nearest.h"
#include "mvhdp_side.h"

namespace {

constexpr int WV = 64;

// ---------------------------------------------------------------------------------------------------------------
// The screen.  Block (b, a) computes the 128 x 128 cells of queries qb0 + 128 a .. against candidates s0 + 128 b .. with screen_tile
// (mvhdp_screen.h has the layout); both images are padded with SCREEN_TILE zero rows.  The stores are checked: cell (i, j) is written
// only for i < q1 and j < s1.
struct ScreenArgs {
    const float* xq; const float* xc;        // the two images, both [.][ld]
    int64_t ld; int kslabs;
    const uint8_t* clsq; const uint8_t* clsc;
    int64_t qb0, q1, s0, s1;                 // the block's queries [qb0, q1) (indices into the query set), the stripe's candidates [s0, s1) (local)
    int excl; int64_t self_delta;            // excl: candidate j is query i itself when j == i + self_delta
    uint32_t* S; int64_t ldS;                // keys [q1 - qb0][ldS], column j - s0
};

__global__ __launch_bounds__(256) void near_screen_kernel(const ScreenArgs p)
{
    const int ta = blockIdx.y, tb = blockIdx.x;
    __shared__ __attribute__((aligned(16))) float As[SCREEN_TILE * SCREEN_LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[SCREEN_TILE * SCREEN_LDS_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64, lr = lane & 31, lh = lane >> 5;
    const int64_t arow0 = p.qb0 + (int64_t)ta * SCREEN_TILE, brow0 = p.s0 + (int64_t)tb * SCREEN_TILE;
    f32x16 acc[2][2];
    screen_tile(p.xq, p.xc, p.ld, p.kslabs, arow0, brow0, As, Bs, acc);

    // epilogue: the 32 lanes of a half write 32 consecutive keys of one query row (128 bytes)
    const int64_t jb = brow0 + wc + lr;                        // + 32 b
    const int64_t ib = arow0 + wr + 4 * lh;                    // + 32 a + (e & 3) + 8 (e >> 2)
    bool cj[2];                                                // the class arrays are padded like the images, with ROW_OUT
#pragma unroll
    for (int b = 0; b < 2; b++) cj[b] = p.clsc[jb + 32 * b] == ROW_TAME;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int64_t i = ib + 32 * a + (e & 3) + 8 * (e >> 2);
            if (i >= p.q1) continue;
            const bool ci = p.clsq[i] == ROW_TAME;
            uint32_t* row = p.S + (i - p.qb0) * p.ldS;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int64_t j = jb + 32 * b;
                if (j < p.s1) row[j - p.s0] =(ci && cj[b] && !(p.excl && j == i + p.self_delta)) ? f32_key(acc[a][b][e]) : 0u;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// One wave per query of the block (a one-wave block, the stripe's keys in LDS).  run_in / run_out [rows][ncap]: the ncap largest keys of
// the stripes so far (rcnt of them).  The cut of this stripe: cells with (double)screen >= (double)tau - margin, tau the ncap-th largest
// key over the stripe's screened cells and run_in; fewer than ncap so far: every screened cell.  A candidate that is not screened
// (ROW_WILD) passes for every query that lists at all; a query that is not screened takes every candidate that may be listed.
constexpr int NEAR_SHORT = 256;                                // keys of a row that the descent may walk from a list of their own

struct SelectArgs {
    const uint32_t* S; int64_t ldS;
    int nrows, ns;                           // queries of the block, candidates of the stripe
    int64_t qb0, s0;
    const uint8_t* clsq; const uint8_t* clsc;
    int excl; int64_t self_delta;
    int ncap; double margin;
    const uint32_t* run_in; const int32_t* rcnt_in; uint32_t* run_out; int32_t* rcnt_out;
    u64* cand; u64 cap; u64* counter;        // entries (row << 32) | local candidate; *counter goes on counting beyond cap
    int32_t* qcount;                         // [rows] candidates of the query over the block's stripes
};

__global__ __launch_bounds__(64) void near_select_kernel(const SelectArgs p)
{
    extern __shared__ uint32_t s_keys[];                       // [ns]
    __shared__ uint32_t s_short[NEAR_SHORT];
    const int lane = threadIdx.x;
    const u64 below = lanes_below(lane);
    for (int r = blockIdx.x; r < p.nrows; r += gridDim.x) {
        const uint8_t cq = p.clsq[p.qb0 + r];
        __syncthreads();                                       // (one wave: the reads of the row before are done)
        for (int w = lane; w < p.ns; w += WV) s_keys[w] = p.S[(int64_t)r * p.ldS + w];
        __syncthreads();
        double cut = -INFINITY;
        if (cq == ROW_TAME) {
            const int rc = p.rcnt_in[r];
            const uint32_t* rin = p.run_in + (int64_t)r * p.ncap;
            uint32_t* rout = p.run_out + (int64_t)r * p.ncap;
            auto count_keys = [&](auto&& test) -> int {
                int c = 0;
                for (int w = lane; w < p.ns; w += WV) c += test(s_keys[w]) ? 1 : 0;
                for (int i = lane; i < rc; i += WV) c += test(rin[i]) ? 1 : 0;
                return wave_sum(c);
            };
            const int nv = count_keys([](uint32_t k) { return k != 0u; });
            uint32_t T = 0u;                                   // keys > T are kept, and need_eq copies of T
            int need_eq = 0;
            if (nv >= p.ncap) {
                // A lower bound first, so that the descent need not walk the whole row 32 times: the ncap-th largest of the 64 lanes' own
                // maxima (where ncap lanes hold a key at all) is reached by at least ncap keys; the keys that reach it -- seldom more than
                // a few times ncap -- go to a short list and the descent runs on that.  More than NEAR_SHORT of them (rows of equal
                // values), or ncap > 64: the descent walks the row.
                uint32_t T0 = 0u;
                if (p.ncap <= WV) {
                    uint32_t lmax = 0u;
                    for (int w = lane; w < p.ns; w += WV) lmax = max(lmax, s_keys[w]);
                    for (int i = lane; i < rc; i += WV) lmax = max(lmax, rin[i]);
                    if (__popcll(ballot(lmax != 0u)) >= p.ncap)
                        T0 = key_descent(0u, 31, [&](uint32_t trial) { return __popcll(ballot(lmax >= trial)) >= p.ncap; });
                }
                int n_short = -1;                              // >= 0: s_short holds every key >= T0, at least ncap of them
                if (T0 != 0u && count_keys([&](uint32_t k) { return k >= T0; }) <= NEAR_SHORT) {
                    n_short = 0;
                    for (int base = 0; base < p.ns + rc; base += WV) {
                        const int w = base + lane;
                        const uint32_t k = w < p.ns ? s_keys[w] : w < p.ns + rc ? rin[w - p.ns] : 0u;
                        const bool in = k >= T0;
                        const u64 m = ballot(in);
                        if (in) s_short[n_short + __popcll(m & below)] = k;
                        n_short += __popcll(m);
                    }
                    __syncthreads();
                }
                auto count_top = [&](auto&& test) -> int {
                    if (n_short < 0) return count_keys(test);
                    int c = 0;
                    for (int i = lane; i < n_short; i += WV) c += test(s_short[i]) ? 1 : 0;
                    return wave_sum(c);
                };
                // the largest T that at least ncap keys reach (>= 1: every screened key is)
                T = key_descent(0u, 31, [&](uint32_t trial) { return count_top([&](uint32_t k) { return k >= trial; }) >= p.ncap; });
                need_eq = p.ncap - count_top([&](uint32_t k) { return k > T; });
                cut = (double)f32_unkey(T) - p.margin;
            }
            int at = 0;
            for (int base = 0; base < p.ns + rc; base += WV) { // the stripe's keys, then the earlier stripes'
                const int w = base + lane;
                const uint32_t k = w < p.ns ? s_keys[w] : w < p.ns + rc ? rin[w - p.ns] : 0u;
                const bool keep = k != 0u && k > T;
                const u64 m = ballot(keep);
                if (keep) rout[at + __popcll(m & below)] = k;
                at += __popcll(m);
            }
            for (int i = lane; i < need_eq; i += WV) rout[at + i] = T;
            if (lane == 0) p.rcnt_out[r] = at + need_eq;       // min(ncap, nv)
        } else if (lane == 0)
            p.rcnt_out[r] = 0;
        if (cq == ROW_OUT) continue;
        const int64_t self = p.excl ? p.qb0 + r + p.self_delta - p.s0 : -1;   // the stripe column of the query itself
        auto passes = [&](int w) -> bool {
            if (w >= p.ns || w == self) return false;
            const uint8_t cj = p.clsc[p.s0 + w];
            if (cq == ROW_WILD) return cj != ROW_OUT;
            const uint32_t k = s_keys[w];
            return cj == ROW_WILD || (k != 0u && (double)f32_unkey(k) >= cut);
        };
        int mine = 0;
        for (int w = lane; w < p.ns; w += WV) mine += passes(w) ? 1 : 0;
        const int total = wave_sum(mine);
        if (total == 0) continue;
        u64 at = 0;
        if (lane == 0) { at = atomicAdd(p.counter, (u64)total); p.qcount[r] += total; }   // (the row is this wave's, the stripes follow one another)
        at = __shfl(at, 0, 64);
        for (int base = 0; base < p.ns; base += WV) {
            const int w = base + lane;
            const bool pass = passes(w);
            const u64 m = ballot(pass);
            const u64 slot = at + (u64)__popcll(m & below);
            if (pass && slot < p.cap) p.cand[slot] = ((u64)r << 32) | (u64)(p.s0 + w);
            at += (u64)__popcll(m);
        }
    }
}

__global__ __launch_bounds__(256) void near_group_kernel(const u64* __restrict__ cand, u64 ncand, const int64_t* __restrict__ qoff, int32_t* __restrict__ qfill, u64* __restrict__ gkey)
{
    const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand) return;
    const u64 key = cand[c];
    const int r = (int)(key >> 32);
    gkey[qoff[r] + atomicAdd(&qfill[r], 1)] = key;
}

// One thread per candidate: the chain of mvhdp_similar_pairs' MVHDP_SIM_COS for (query, candidate).
__global__ __launch_bounds__(256) void near_exact_kernel(const double* __restrict__ q, const double* __restrict__ qnorm, int64_t qb0, const double* __restrict__ x,
                                                         const double* __restrict__ xnorm, int dim, const u64* __restrict__ gkey, u64 ncand, double* __restrict__ gsim)
{
    const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand) return;
    const u64 key = gkey[c];
    const int64_t i = qb0 + (int64_t)(key >> 32), j = (int64_t)(key & 0xffffffffull);
    gsim[c] = screen_exact_dot(q + i * dim, x + j * dim, dim) / (qnorm[i] * xnorm[j]);   // dot / (twoNorm * twoNorm)
}

// ---------------------------------------------------------------------------------------------------------------
// One wave per query: the first n_cap of its candidates by (sim descending, local id ascending); a NaN sim does not count.
__global__ __launch_bounds__(64) void near_pick_kernel(const u64* __restrict__ gkey, const double* __restrict__ gsim, const int64_t* __restrict__ qoff, int nrows, int n_cap,
                                                       u64* __restrict__ sel_hi, uint32_t* __restrict__ sel_lo, int32_t* __restrict__ out_id, double* __restrict__ out_sim,
                                                       int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int64_t b = qoff[r], m = qoff[r + 1] - b;
        int32_t* oi = out_id + (int64_t)r * n_cap;
        double* os = out_sim + (int64_t)r * n_cap;
        const int n_eff = wave_first_n(
            [&](int64_t i, u64& h, uint32_t& l) { const double v = gsim[b + i]; h = v != v ? 0ull : f64_key(v); l = ~(uint32_t)(gkey[b + i] & 0xffffffffull); },
            m, n_cap, lane, sel_hi + (int64_t)r * n_cap, sel_lo + (int64_t)r * n_cap,
            [&](int place, u64 h, uint32_t l) { oi[place] = (int32_t)~l; os[place] = f64_unkey(h); });
        if (lane == 0) counts[r] = n_eff;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// mvhdp_topic_top_entities.  prop: [nd][K] proportions of a chunk.  Thread (slice, k), k fastest, walks the entities of its slice in id
// order and keeps the n largest prop[.][k] > threshold as an unordered set: lists [slice][n][K] (k fastest: a wave's reads of prop and its
// list accesses are rows of consecutive topics), id -1 in an unused place.  An equal weight never displaces an earlier entity.
__global__ __launch_bounds__(256) void topk_partial_kernel(const double* __restrict__ prop, int64_t nd, int K, int64_t slice_len, int64_t nslices, int n, double threshold,
                                                           int32_t id0, double* __restrict__ pw, int32_t* __restrict__ pid)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nslices * K) return;
    const int64_t sl = t / K;
    const int k = (int)(t - sl * K);
    double* w = pw + sl * n * K + k;
    int32_t* id = pid + sl * n * K + k;
    const int64_t dend = (sl + 1) * slice_len < nd ? (sl + 1) * slice_len : nd;
    int cnt = 0, pmin = 0;
    double wmin = 0.0;                                         // the set's last member in the order: smallest weight, among equals the largest id
    for (int64_t d = sl * slice_len; d < dend; d++) {
        const double v = prop[d * K + k];
        if (!(v > threshold)) continue;
        if (cnt < n) {
            w[(int64_t)cnt * K] = v; id[(int64_t)cnt * K] = id0 + (int32_t)d;
            if (cnt == 0 || v <= wmin) { wmin = v; pmin = cnt; }
            cnt++;
        } else if (v > wmin) {
            w[(int64_t)pmin * K] = v; id[(int64_t)pmin * K] = id0 + (int32_t)d;
            wmin = w[0]; pmin = 0;
            for (int j = 1; j < n; j++) {
                const double x = w[(int64_t)j * K];
                if (x < wmin || (x == wmin && id[(int64_t)j * K] > id[(int64_t)pmin * K])) { wmin = x; pmin = j; }
            }
        }
    }
    for (int j = cnt; j < n; j++) { w[(int64_t)j * K] = 0.0; id[(int64_t)j * K] = -1; }
}

// One wave per topic over the lists of every slice: entries i = 0 .. entries - 1 at [i][K].
__global__ __launch_bounds__(64) void topk_merge_kernel(const double* __restrict__ pw, const int32_t* __restrict__ pid, int64_t entries, int K, int n,
                                                        u64* __restrict__ sel_hi, uint32_t* __restrict__ sel_lo, int32_t* __restrict__ out_id, double* __restrict__ out_w,
                                                        int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        int32_t* oi = out_id + (int64_t)k * n;
        double* ow = out_w + (int64_t)k * n;
        const int n_eff = wave_first_n(
            [&](int64_t i, u64& h, uint32_t& l) { const int32_t e = pid[i * K + k]; h = e < 0 ? 0ull : f64_key(pw[i * K + k]); l = ~(uint32_t)e; },
            entries, n, lane, sel_hi + (int64_t)k * n, sel_lo + (int64_t)k * n,
            [&](int place, u64 h, uint32_t l) { oi[place] = (int32_t)~l; ow[place] = f64_unkey(h); });
        if (lane == 0) counts[k] = n_eff;
    }
}

// the proportions of entities [d0, d1) into out [d1 - d0][K], chunk by chunk
int launch_theta(mvhdp_ctx* h, const DocTopicCarry& carry, const double* d_w, int64_t d0, int64_t d1, double* out)
{
    const int K = h->mm.K;
    const int64_t chunk = near_chunk(K, 0);
    for (int64_t a = d0; a < d1; a += chunk)
        HIPC(h, mvhdp_launch_doc_topic_prop(h->mm, carry, d_w, a, std::min(a + chunk, d1), out + (a - d0) * K, h->stream));
    return MVHDP_OK;
}

} // namespace

// ---------------------------------------------------------------------------------------------------------------
extern "C" int mvhdp_nearest_probe(int64_t nq, int64_t nc, int32_t K, int32_t block_queries, int32_t stripe_candidates, mvhdp_nearest_stats* out)
{
    if (!out || nq < 0 || nc < 0 || K < 1 || block_queries < 0 || stripe_candidates < 0) return MVHDP_ERR_INVALID_ARG;
    if (K > SIM_MAX_DIM) return MVHDP_ERR_UNSUPPORTED;
    memset(out, 0, sizeof *out);
    out->margin = sim_margin(K);
    out->blocks = (int32_t)near_blocks(nq, nc, block_queries, stripe_candidates);
    out->cells_screened = near_cells(nq, nc, block_queries, stripe_candidates);
    return MVHDP_OK;
}

extern "C" int mvhdp_nearest_entities(mvhdp_handle h, const mvhdp_nearest_args* a, int64_t* ids, double* sims, int32_t* counts, mvhdp_nearest_stats* stats)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (!a || !ids || !sims || !counts) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: null arguments or a null output");
    if (!a->view_weights) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: null view_weights");
    if (a->n < 1) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: n < 1");
    if (a->c0 < 0 || a->c1 > mm.D || a->c0 > a->c1) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: bad candidate range");
    if (a->queries ? a->nq < 0 : (a->q0 < 0 || a->q1 > mm.D || a->q0 > a->q1)) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: bad query range or negative nq");
    if (a->min_weight != a->min_weight) FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: min_weight is NaN");
    if (a->block_queries < 0 || a->stripe_candidates < 0 || a->candidate_capacity < 0)
        FAIL(h, MVHDP_ERR_INVALID_ARG, "nearest_entities: negative block_queries, stripe_candidates or candidate_capacity");
    if (K > SIM_MAX_DIM) FAIL(h, MVHDP_ERR_UNSUPPORTED, "nearest_entities: K > 65536 (the screen's margin would reach 0.01)");
    const int64_t nq = a->queries ? a->nq : a->q1 - a->q0, C = a->c1 - a->c0;
    if (nq >= ((int64_t)1 << 31) - SCREEN_TILE || C >= ((int64_t)1 << 31) - SCREEN_TILE) FAIL(h, MVHDP_ERR_UNSUPPORTED, "nearest_entities: 2^31 rows or more");
    DocTopicCarry carry{};
    int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
    const int n = a->n;
    mvhdp_nearest_stats st{};
    st.margin = sim_margin(K);
    st.blocks = (int32_t)near_blocks(nq, C, a->block_queries, a->stripe_candidates);
    st.cells_screened = near_cells(nq, C, a->block_queries, a->stripe_candidates);
    std::vector<int64_t> r_ids((size_t)nq * n, -1);
    std::vector<double> r_sims((size_t)nq * n, 0.0);
    std::vector<int32_t> r_counts((size_t)nq, 0);
    auto deliver = [&]() {
        memcpy(ids, r_ids.data(), r_ids.size() * sizeof(int64_t));
        memcpy(sims, r_sims.data(), r_sims.size() * sizeof(double));
        memcpy(counts, r_counts.data(), r_counts.size() * sizeof(int32_t));
        if (stats) *stats = st;
        return MVHDP_OK;
    };
    if (nq == 0 || C == 0) return deliver();
    HIPC(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;

    // the two sets of rows, on the device for the whole call: 12 bytes per entry (fp64 rows for the exact stage, their fp32 image for the screen)
    const int64_t ld = screen_ld(K);
    DevArray<double> d_w;
    ScreenRows qr, cr;
    HIPC(h, d_w.alloc((size_t)mm.M));
    HIPC(h, d_w.upload(a->view_weights, (size_t)mm.M, s));
    HIPC(h, cr.x.alloc((size_t)C * K));
    HIPC(h, qr.x.alloc((size_t)nq * K));
    rc = launch_theta(h, carry, d_w, a->c0, a->c1, cr.x); if (rc) return rc;
    if (a->queries) HIPC(h, qr.x.upload(a->queries, (size_t)nq * K, s));
    else { rc = launch_theta(h, carry, d_w, a->q0, a->q1, qr.x); if (rc) return rc; }
    rc = mvhdp_screen_prepare_rows(h, cr, C, K, a->min_weight, SCREEN_TILE, true); if (rc) return rc;
    rc = mvhdp_screen_prepare_rows(h, qr, nq, K, a->min_weight, SCREEN_TILE, true); if (rc) return rc;
    {
        std::vector<uint8_t> hc((size_t)std::max(nq, C));
        for (const ScreenRows* r : {&qr, &cr}) {
            const size_t cnt = (size_t)(r == &qr ? nq : C);
            HIPC(h, hipMemcpyAsync(hc.data(), r->cls.get(), cnt, hipMemcpyDeviceToHost, s));
            HIPC(h, hipStreamSynchronize(s));
            for (size_t i = 0; i < cnt; i++) st.exact_only_rows += hc[i] == ROW_WILD ? 1 : 0;
        }
    }

    const int64_t B = std::min(near_block(a->block_queries, a->stripe_candidates), nq), S = std::min(near_stripe(a->stripe_candidates), C);
    const int ncap = (int)std::min<int64_t>(n, C);
    const int excl = (!a->queries && a->exclude_self) ? 1 : 0;
    const int64_t self_delta = a->queries ? 0 : a->q0 - a->c0;
    u64 ccap = (u64)(a->candidate_capacity > 0 ? a->candidate_capacity : NEAR_AUTO_CAPACITY);
    DevArray<uint32_t> d_S, d_run[2], d_sello;
    DevArray<int32_t> d_rcnt[2], d_qcount, d_qfill, d_oid, d_cnt;
    DevArray<u64> d_ctr, d_cand, d_gkey, d_selhi;
    DevArray<double> d_gsim, d_osim;
    DevArray<int64_t> d_qoff;
    HIPC(h, d_S.alloc((size_t)B * S));
    for (int i = 0; i < 2; i++) { HIPC(h, d_run[i].alloc((size_t)B * ncap)); HIPC(h, d_rcnt[i].alloc((size_t)B)); }
    HIPC(h, d_sello.alloc((size_t)B * ncap));
    HIPC(h, d_selhi.alloc((size_t)B * ncap));
    HIPC(h, d_oid.alloc((size_t)B * ncap));
    HIPC(h, d_osim.alloc((size_t)B * ncap));
    HIPC(h, d_qcount.alloc((size_t)B));
    HIPC(h, d_qfill.alloc((size_t)B));
    HIPC(h, d_cnt.alloc((size_t)B));
    HIPC(h, d_qoff.alloc((size_t)B + 1));
    HIPC(h, d_ctr.alloc(1));
    auto size_buffers = [&](u64 c) -> hipError_t {
        hipError_t e = d_cand.alloc((size_t)c);
        if (e == hipSuccess) e = d_gkey.alloc((size_t)c);
        if (e == hipSuccess) e = d_gsim.alloc((size_t)c);
        return e;
    };
    HIPC(h, size_buffers(ccap));
    std::vector<int32_t> h_qcount((size_t)B), h_oid((size_t)B * ncap), h_cnt((size_t)B);
    std::vector<int64_t> h_qoff((size_t)B + 1);
    std::vector<double> h_osim((size_t)B * ncap);

    for (int64_t qb0 = 0; qb0 < nq; qb0 += B) {
        const int64_t q1 = std::min(qb0 + B, nq), nr = q1 - qb0;
        u64 ncand = 0;
        for (int attempt = 0; ; attempt++) {
            HIPC(h, d_ctr.fill(0, s));
            HIPC(h, d_qcount.fill(0, s));
            HIPC(h, d_rcnt[0].fill(0, s));
            int flip = 0;
            for (int64_t s0 = 0; s0 < C; s0 += S, flip ^= 1) {
                const int64_t s1 = std::min(s0 + S, C);
                ScreenArgs sa{};
                sa.xq = qr.xn; sa.xc = cr.xn; sa.ld = ld; sa.kslabs = (int)(ld / SCREEN_BK); sa.clsq = qr.cls; sa.clsc = cr.cls;
                sa.qb0 = qb0; sa.q1 = q1; sa.s0 = s0; sa.s1 = s1; sa.excl = excl; sa.self_delta = self_delta; sa.S = d_S; sa.ldS = S;
                LAUNCH(h, near_screen_kernel, dim3((unsigned)near_tiles(s1 - s0), (unsigned)near_tiles(nr)), dim3(256), 0, s, sa);
                SelectArgs se{};
                se.S = d_S; se.ldS = S; se.nrows = (int)nr; se.ns = (int)(s1 - s0); se.qb0 = qb0; se.s0 = s0; se.clsq = qr.cls; se.clsc = cr.cls;
                se.excl = excl; se.self_delta = self_delta; se.ncap = ncap; se.margin = st.margin;
                se.run_in = d_run[flip]; se.rcnt_in = d_rcnt[flip]; se.run_out = d_run[flip ^ 1]; se.rcnt_out = d_rcnt[flip ^ 1];
                se.cand = d_cand; se.cap = ccap; se.counter = d_ctr; se.qcount = d_qcount;
                LAUNCH(h, near_select_kernel, dim3(row_blocks(nr, h->num_cus)), dim3(WV), (size_t)(s1 - s0) * sizeof(uint32_t), s, se);
            }
            HIPC(h, d_ctr.download(&ncand, 1, s));
            HIPC(h, d_qcount.download(h_qcount.data(), (size_t)nr, s));
            HIPC(h, hipStreamSynchronize(s));
            if (ncand <= ccap) break;
            if (attempt) FAIL(h, MVHDP_ERR_HIP, "nearest_entities: a block asked for more room twice");   // the count is a function of the data alone
            ccap = ncand;                                      // redo the block with the room it asked for
            st.regrown++;
            HIPC(h, size_buffers(ccap));
        }
        st.candidates += (int64_t)ncand;
        if (ncand == 0) continue;
        h_qoff[0] = 0;
        for (int64_t r = 0; r < nr; r++) h_qoff[(size_t)r + 1] = h_qoff[(size_t)r] + h_qcount[(size_t)r];
        HIPC(h, d_qoff.upload(h_qoff.data(), (size_t)nr + 1, s));
        HIPC(h, d_qfill.fill(0, s));
        const unsigned cblocks = (unsigned)((ncand + 255) / 256);
        LAUNCH(h, near_group_kernel, dim3(cblocks), dim3(256), 0, s, d_cand, ncand, d_qoff, d_qfill, d_gkey);
        LAUNCH(h, near_exact_kernel, dim3(cblocks), dim3(256), 0, s, qr.x, qr.norm, qb0, cr.x, cr.norm, K, d_gkey, ncand, d_gsim);
        LAUNCH(h, near_pick_kernel, dim3(row_blocks(nr, h->num_cus)), dim3(WV), 0, s, d_gkey, d_gsim, d_qoff, (int)nr, ncap, d_selhi, d_sello, d_oid, d_osim, d_cnt);
        HIPC(h, d_oid.download(h_oid.data(), (size_t)nr * ncap, s));
        HIPC(h, d_osim.download(h_osim.data(), (size_t)nr * ncap, s));
        HIPC(h, d_cnt.download(h_cnt.data(), (size_t)nr, s));
        HIPC(h, hipStreamSynchronize(s));
        for (int64_t r = 0; r < nr; r++) {
            const int c = h_cnt[(size_t)r];
            r_counts[(size_t)(qb0 + r)] = c;
            for (int i = 0; i < c; i++) {
                r_ids[(size_t)(qb0 + r) * n + i] = a->c0 + h_oid[(size_t)r * ncap + i];
                r_sims[(size_t)(qb0 + r) * n + i] = h_osim[(size_t)r * ncap + i];
            }
        }
    }
    return deliver();
}

extern "C" int mvhdp_topic_top_entities(mvhdp_handle h, const double* view_weights, int64_t d0, int64_t d1, int32_t n, double threshold,
                                        int64_t chunk_entities, int64_t slice_entities, int64_t* ids, double* weights, int32_t* counts)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (!view_weights || !ids || !weights || !counts) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_top_entities: null view_weights or a null output");
    if (d0 < 0 || d1 > mm.D || d0 > d1) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_top_entities: bad entity range");
    if (n < 1 || n > NEAR_MAX_TOPN) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_top_entities: n outside 1..1024");
    if (threshold != threshold) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_top_entities: threshold is NaN");
    if (chunk_entities < 0 || slice_entities < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_top_entities: negative chunk_entities or slice_entities");
    const int64_t nd = d1 - d0;
    if (nd >= (int64_t)1 << 31) FAIL(h, MVHDP_ERR_UNSUPPORTED, "topic_top_entities: 2^31 entities or more");
    DocTopicCarry carry{};
    int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
    std::vector<int32_t> h_id((size_t)K * n, -1), h_cnt((size_t)K, 0);
    std::vector<double> h_w((size_t)K * n, 0.0);
    if (nd > 0) {
        HIPC(h, hipSetDevice(h->device));
        hipStream_t s = h->stream;
        const int64_t chunk = near_chunk(K, chunk_entities), slice = near_slice(slice_entities), nsl = near_slices(nd, K, chunk_entities, slice_entities);
        DevArray<double> d_w, d_prop, d_pw, d_ow;
        DevArray<int32_t> d_pid, d_oid, d_cnt;
        DevArray<u64> d_selhi;
        DevArray<uint32_t> d_sello;
        HIPC(h, d_w.alloc((size_t)mm.M));
        HIPC(h, d_prop.alloc((size_t)std::min(chunk, nd) * K));
        HIPC(h, d_pw.alloc((size_t)nsl * n * K));
        HIPC(h, d_pid.alloc((size_t)nsl * n * K));
        HIPC(h, d_ow.alloc((size_t)K * n));
        HIPC(h, d_oid.alloc((size_t)K * n));
        HIPC(h, d_cnt.alloc((size_t)K));
        HIPC(h, d_selhi.alloc((size_t)K * n));
        HIPC(h, d_sello.alloc((size_t)K * n));
        HIPC(h, d_w.upload(view_weights, (size_t)mm.M, s));
        int64_t sl0 = 0;
        for (int64_t c0 = 0; c0 < nd; c0 += chunk) {
            const int64_t c1 = std::min(c0 + chunk, nd), ns = (c1 - c0 + slice - 1) / slice;
            HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, d_w, d0 + c0, d0 + c1, d_prop, s));
            LAUNCH(h, topk_partial_kernel, dim3((unsigned)((ns * K + 255) / 256)), dim3(256), 0, s, d_prop, c1 - c0, K, slice, ns, (int)n, threshold, (int32_t)c0,
                   d_pw + sl0 * n * K, d_pid + sl0 * n * K);
            sl0 += ns;
        }
        LAUNCH(h, topk_merge_kernel, dim3(row_blocks(K, h->num_cus)), dim3(WV), 0, s, d_pw, d_pid, nsl * n, K, (int)n, d_selhi, d_sello, d_oid, d_ow, d_cnt);
        HIPC(h, d_oid.download(h_id.data(), (size_t)K * n, s));
        HIPC(h, d_ow.download(h_w.data(), (size_t)K * n, s));
        HIPC(h, d_cnt.download(h_cnt.data(), (size_t)K, s));
        HIPC(h, hipStreamSynchronize(s));
    }
    for (int k = 0; k < K; k++) {
        counts[k] = h_cnt[(size_t)k];
        for (int i = 0; i < n; i++) {
            const bool have = i < h_cnt[(size_t)k];
            ids[(size_t)k * n + i] = have ? d0 + h_id[(size_t)k * n + i] : -1;
            weights[(size_t)k * n + i] = have ? h_w[(size_t)k * n + i] : 0.0;
        }
    }
    return MVHDP_OK;
}
