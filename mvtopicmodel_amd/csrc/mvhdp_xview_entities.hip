// mvhdp_xview_entities.hip — cross-view prediction from the item's side: rank the candidate entities of [c0, c1) per query by
// score(d, j) = sum_k theta_d[k] * psi_j[k], psi_j a weighted set of phi rows of view m or a host row (include/mvhdp.h has the contract:
// the chains, the order, the excluded set; tests/native/xview_entities_ref.c restates it on the host).
//   xe_psi_kernel         psi_j[k] = the chain p = fma(c_i, phi[w_i][k], p) over the query's items, phi formed in place by the expression
//                         of xview_phi_kernel: one thread per (query, topic), the count rows read K-contiguously.
//   xview_score_kernel    (mvhdp_xview.h) with the roles swapped: psi in the theta slot, a block of theta rows in the phi slot; the block
//                         of scores is [queries of the block][entities of the block], a query's row contiguous over entities.
//   xe_pair_score_kernel  one thread per pair: the plain chain over the pair's theta row and psi row, nothing marked yet.
//   xe_mark_kernel        one wave per entity of the block walks its view-m span; for every token the queries that hold that type (a
//                         type-to-queries list the host builds per block of queries) get the marker whose key is 0 at S[query][entity].
//                         An integer exchange, so that a cell marked twice is counted once.
//   xe_pick_kernel        one wave per query: the first n of (the block's cells that are not marked, the n carried from the blocks
//                         before) by (score key descending, entity ascending): wave_first_n (mvhdp_select.h) on the composite (key,
//                         ~candidate).  The block's keys are staged in LDS while a row fits 64 KiB (8192 entities); beyond that the
//                         passes read the block of scores where it lies.  Once n are carried, only a cell in front of the last carried
//                         entry can enter: the row is read once, those cells are compacted, and while they and the carried ones are
//                         at most 256 the wave holds them in registers (four a lane) and places each by counting, without a descent.
//   xe_rank_kernel        one wave per pair: the cells of its query's row that are not marked, the queried entity apart, and precede
//                         (score, entity) (wave_rank_count of mvhdp_select.h); the counts add over the blocks of entities.
// Work is cut on the host: queries in blocks, entities in blocks, the block of scores within 256 MiB.  theta is formed per block of
// entities (mvhdp_launch_doc_topic_prop) and never leaves the device.  No floating-point atomics; everything runs on the handle's stream.
#include "mvhdp_side.h"
#include "mvhdp_select.h"
#include "mvhdp_xview.h"

namespace {

constexpr int64_t XE_BLOCK_CELLS = ((int64_t)256 << 20) / (int64_t)sizeof(double);   // the block of scores: at most 256 MiB
constexpr int64_t XE_LDS_ENTITIES = 8192;                      // a query's row of keys up to this many entities is selected from LDS (64 KiB)
constexpr int64_t XE_AUTO_QUERIES = 4096;
constexpr int XE_MAX_N = 1024;
constexpr int XE_SHORT_T = 4, XE_SHORT = 64 * XE_SHORT_T;      // entries a wave places from registers: four a lane
constexpr int64_t XE_MAX_QUERY_ITEMS = (int64_t)1 << 20;
constexpr double XE_MAX_WEIGHT = 9007199254740992.0;           // 2^53

// q_list: the query of row j (nullptr: q_first + j); q_off / q_items / q_w: the whole call's
__global__ __launch_bounds__(256) void xe_psi_kernel(const int32_t* __restrict__ rows /*n_wk of view m*/, const int32_t* __restrict__ nk, const uint8_t* __restrict__ inactive,
                                                     int K, int64_t n_rows, const int64_t* __restrict__ q_list, int64_t q_first, const int64_t* __restrict__ q_off,
                                                     const int32_t* __restrict__ q_items, const double* __restrict__ q_w, double beta, double beta_sum, double* __restrict__ psi)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_rows * K) return;
    const int64_t j = t / K;
    const int k = (int)(t - j * K);
    const int64_t q = q_list ? q_list[j] : q_first + j;
    const bool off = inactive[k] != 0;
    double p = 0.0;
    for (int64_t i = q_off[q]; i < q_off[q + 1]; i++) {
        const double phi = off ? 0.0 : ((double)rows[(int64_t)q_items[i] * K + k] + beta) / ((double)nk[k] + beta_sum);
        p = __builtin_fma(q_w ? q_w[i] : 1.0, phi, p);
    }
    psi[t] = p;
}

// pair p: query row pair_row[p] of the block of queries, candidate pair_ent[p] (an index into [c0, c1)) inside the block of entities at e0
__global__ __launch_bounds__(256) void xe_pair_score_kernel(const double* __restrict__ theta, const double* __restrict__ psi, int K, int64_t n_pairs,
                                                            const int32_t* __restrict__ pair_row, const uint32_t* __restrict__ pair_ent, uint32_t e0, double* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const double* __restrict__ th = theta + (int64_t)(pair_ent[p] - e0) * K;
    const double* __restrict__ ps = psi + (int64_t)pair_row[p] * K;
    double s = 0.0;
    for (int k = 0; k < K; k++) s = __builtin_fma(th[k], ps[k], s);
    out[p] = s;
}

// column e of the block is entity d0 + e of the handle
__global__ __launch_bounds__(256) void xe_mark_kernel(u64* __restrict__ S, int64_t ld, int64_t ne, int64_t d0, int64_t V, const int64_t* __restrict__ doc_off,
                                                      const int32_t* __restrict__ tok, const int64_t* __restrict__ inv_off /*[V + 1]*/, const int32_t* __restrict__ inv_q,
                                                      u64* __restrict__ n_marked)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    int c = 0;
    for (int64_t e = wave; e < ne; e += nwaves) {
        const int64_t b = doc_off[d0 + e], en = doc_off[d0 + e + 1];
        for (int64_t i = b + lane; i < en; i += 64) {
            const int32_t w = tok[i];
            if (w < 0 || (int64_t)w >= V) continue;
            for (int64_t j = inv_off[w]; j < inv_off[w + 1]; j++)
                c += atomicExch(&S[(int64_t)inv_q[j] * ld + e], XV_EXCLUDED) != XV_EXCLUDED ? 1 : 0;
        }
    }
    c = wave_sum(c);
    if (lane == 0 && c) atomicAdd(n_marked, (u64)c);
}

struct PickArgs {
    const u64* S; int64_t ld;                // the block of scores, read as bits
    int nrows, ne;                           // queries of the block, entities of the block
    uint32_t e0;                             // column 0 is candidate e0 of [c0, c1)
    int n_cap;
    const u64* in_hi; const uint32_t* in_lo; const int32_t* in_cnt;   // [rows][n_cap]: the first n of the blocks before, in order (key, ~candidate)
    u64* out_hi; uint32_t* out_lo; int32_t* out_cnt;                  // ... with this block
    u64* sel_hi; uint32_t* sel_lo; int sel_pitch;                     // [rows][sel_pitch] scratch, sel_pitch >= max(n_cap, XE_SHORT)
};

// One wave per query (the block is this one wave).  Entries: the block's ne cells, then the in_cnt carried ones; an entry counts when its
// key is not 0; the composites (key, ~candidate) of the entries that count are distinct.
template <bool IN_LDS>
__global__ __launch_bounds__(64) void xe_pick_kernel(const PickArgs p)
{
    extern __shared__ u64 s_keys[];                            // IN_LDS: [ne]
    const int lane = threadIdx.x;
    const u64 below = lanes_below(lane);
    for (int r = blockIdx.x; r < p.nrows; r += gridDim.x) {
        const u64* __restrict__ row = p.S + (int64_t)r * p.ld;
        const int rc = p.in_cnt[r], m = p.ne + rc;
        const u64* __restrict__ ih = p.in_hi + (int64_t)r * p.n_cap;
        const uint32_t* __restrict__ il = p.in_lo + (int64_t)r * p.n_cap;
        u64* __restrict__ sh = p.sel_hi + (int64_t)r * p.sel_pitch;
        uint32_t* __restrict__ sl = p.sel_lo + (int64_t)r * p.sel_pitch;
        u64* __restrict__ oh = p.out_hi + (int64_t)r * p.n_cap;
        uint32_t* __restrict__ ol = p.out_lo + (int64_t)r * p.n_cap;
        if (rc == p.n_cap) {
            // The carry is full and in order: a cell behind its last entry has n_cap entries in front of it and cannot be listed.
            const u64 fh = ih[rc - 1]; const uint32_t fl = il[rc - 1];
            int ns = 0;
            for (int base = 0; base < p.ne; base += 64) {
                const int i = base + lane;
                u64 h = 0; uint32_t l = 0;
                if (i < p.ne) { h = f64_bits_key(row[i]); l = ~(p.e0 + (uint32_t)i); }
                const bool in = h != 0 && (h > fh || (h == fh && l > fl));
                const u64 mk = ballot(in);
                if (in) { const int pos = ns + __popcll(mk & below); if (pos < XE_SHORT) { sh[pos] = h; sl[pos] = l; } }
                ns += __popcll(mk);
            }
            if (ns == 0) {                                     // nothing enters: the carry as it is
                for (int i = lane; i < rc; i += 64) { oh[i] = ih[i]; ol[i] = il[i]; }
                if (lane == 0) p.out_cnt[r] = rc;
                continue;
            }
            const int mt = ns + rc;
            if (mt <= XE_SHORT) {
                __syncthreads();                               // the wave reads what its other lanes wrote
                u64 eh[XE_SHORT_T]; uint32_t el[XE_SHORT_T]; int place[XE_SHORT_T];
#pragma unroll
                for (int t = 0; t < XE_SHORT_T; t++) {         // entry lane + 64 t: the cells that may enter, then the carried
                    const int j = lane + 64 * t;
                    eh[t] = j < ns ? sh[j] : j < mt ? ih[j - ns] : 0ull;
                    el[t] = j < ns ? sl[j] : j < mt ? il[j - ns] : 0u;
                    place[t] = 0;
                }
#pragma unroll
                for (int t = 0; t < XE_SHORT_T; t++) {
                    const int nt = mt - 64 * t < 64 ? mt - 64 * t : 64;   // (wave-uniform)
                    for (int src = 0; src < nt; src++) {
                        const u64 bh = ((u64)(uint32_t)__shfl((int)(eh[t] >> 32), src, 64) << 32) | (u64)(uint32_t)__shfl((int)(uint32_t)eh[t], src, 64);
                        const uint32_t bl = (uint32_t)__shfl((int)el[t], src, 64);
#pragma unroll
                        for (int u = 0; u < XE_SHORT_T; u++) place[u] += (bh > eh[u] || (bh == eh[u] && bl > el[u])) ? 1 : 0;
                    }
                }
#pragma unroll
                for (int t = 0; t < XE_SHORT_T; t++)
                    if (eh[t] != 0 && place[t] < p.n_cap) { oh[place[t]] = eh[t]; ol[place[t]] = el[t]; }
                if (lane == 0) p.out_cnt[r] = p.n_cap;         // mt > n_cap entries that count
                __syncthreads();                               // (the scratch is free for the row after next that this wave takes)
                continue;
            }
        }
        if (IN_LDS) {
            __syncthreads();                                   // (one wave: the reads of the row before are done)
            for (int w = lane; w < p.ne; w += 64) s_keys[w] = f64_bits_key(row[w]);
            __syncthreads();
        }
        const int n_eff = wave_first_n(
            [&](int i, u64& h, uint32_t& l) {
                if (i < p.ne) { h = IN_LDS ? s_keys[i] : f64_bits_key(row[i]); l = ~(p.e0 + (uint32_t)i); }
                else { h = ih[i - p.ne]; l = il[i - p.ne]; }
            },
            m, p.n_cap, lane, sh, sl, [&](int place, u64 h, uint32_t l) { oh[place] = h; ol[place] = l; });
        if (lane == 0) p.out_cnt[r] = n_eff;
    }
}

__global__ __launch_bounds__(256) void xe_rank_kernel(const u64* __restrict__ S, int64_t ld, int ne, uint32_t e0, int64_t n_pairs, const int32_t* __restrict__ pair_row,
                                                      const uint32_t* __restrict__ pair_ent, const u64* __restrict__ pair_score, u64* __restrict__ rank)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t p = wave; p < n_pairs; p += nwaves) {
        const int c = wave_rank_count(S + (int64_t)pair_row[p] * ld, ne, e0, f64_bits_key(pair_score[p]), pair_ent[p], lane);
        if (lane == 0) rank[p] += (u64)c;                      // the pair is this wave's; the blocks follow one another on the stream
    }
}

struct EntPredict {
    int32_t n = 0;
    std::vector<int64_t> ids;
    std::vector<double> scores;
    std::vector<int32_t> counts;
};

struct EntRank {
    int64_t n = 0;
    const int64_t* query = nullptr;
    const int64_t* entity = nullptr;
    std::vector<double> score;
    std::vector<int64_t> rank;
};

// the arguments both calls share; every check comes before the first output is touched
int check_args(mvhdp_ctx* h, const mvhdp_entities_args* a, const char* who)
{
    MvModel& mm = h->mm;
    const std::string w(who);
    if (!a) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": null arguments");
    if (a->m < 0 || a->m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": bad view");
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, w + " before set_hyper");
    rc = require_current_counts(h, w); if (rc) return rc;
    if (a->c0 < 0 || a->c1 > mm.D || a->c0 > a->c1) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": bad candidate range");
    if (a->nq < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": negative nq");
    if (a->block_entities < 0 || a->block_queries < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": negative block_entities or block_queries");
    if (const char* r = check_view_weights(a->view_weights, mm.M)) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": " + r);
    if (a->psi) {
        if (const char* r = check_nonneg_finite(a->psi, a->nq * mm.K)) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": a psi entry " + r);
    } else if (a->nq > 0) {
        if (!a->q_off) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": null q_off");
        if (const char* r = check_offsets(a->q_off, a->nq, XE_MAX_QUERY_ITEMS)) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": q_off (a query: at most 2^20 items) " + r);
        const int64_t total = a->q_off[a->nq];
        if (total > 0 && !a->q_items) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": null q_items");
        const int32_t V = mm.V[a->m];
        for (int64_t i = 0; i < total; i++) {
            if (a->q_items[i] < 0 || a->q_items[i] >= V) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": a query item outside the view's types");
            if (a->q_weights && (!(a->q_weights[i] >= 0.0) || !(a->q_weights[i] <= XE_MAX_WEIGHT))) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": a query weight outside [0, 2^53]");
        }
    }
    if (a->c1 - a->c0 >= (int64_t)1 << 31) FAIL(h, MVHDP_ERR_UNSUPPORTED, w + ": 2^31 candidates or more");
    return MVHDP_OK;
}

// The work of both calls.  rk: score and rank the pairs; else pr: the first pr->n candidates of every query.
int entities_run(mvhdp_ctx* h, const mvhdp_entities_args* a, EntPredict* pr, EntRank* rk, mvhdp_entities_stats& st)
{
    MvModel& mm = h->mm;
    const int K = mm.K, m = a->m;
    const int64_t V = mm.V[m], C = a->c1 - a->c0;
    const bool item_form = a->psi == nullptr, excl = item_form && a->exclude_present != 0;
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    // the queries that take part: every one (predict), or those that have pairs, each once (rank)
    std::vector<int64_t> qsel, order;
    if (rk) {
        qsel.assign(rk->query, rk->query + rk->n);
        std::sort(qsel.begin(), qsel.end());
        qsel.erase(std::unique(qsel.begin(), qsel.end()), qsel.end());
    }
    const int64_t nqs = rk ? (int64_t)qsel.size() : a->nq;

    // the sizes of the cuts
    int64_t BE = a->block_entities > 0 ? a->block_entities : XE_LDS_ENTITIES;
    BE = std::min(BE, std::max<int64_t>(1, XE_BLOCK_CELLS / K));                  // the block's theta rows stay within 256 MiB as well
    BE = std::max<int64_t>(1, std::min(BE, C));
    int64_t BQ = a->block_queries > 0 ? a->block_queries : XE_AUTO_QUERIES;
    BQ = std::max<int64_t>(1, std::min(std::min(BQ, XE_BLOCK_CELLS / BE), nqs));
    BQ = std::min(BQ, std::max<int64_t>(1, XE_BLOCK_CELLS / K));

    DocTopicCarry carry{};
    int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
    const int32_t* d_rows = mm.counts + mm.rowbase[m] * K;
    const int32_t* d_nk = mm.counts + mm.rowbase[mm.M] * K + (int64_t)m * K;
    const int n_cap = pr ? (int)std::min<int64_t>(pr->n, C) : 0, sel_pitch = std::max(n_cap, XE_SHORT);

    DevArray<double> d_w, d_theta, d_psi, d_S, d_qw, d_pscore;     // d_S and d_pscore are also read as u64 keys
    DevArray<int64_t> d_qoff, d_qlist, d_invoff;
    DevArray<int32_t> d_qitems, d_invq, d_cnt[2], d_prow;
    DevArray<uint32_t> d_lo[2], d_sello, d_pent;
    DevArray<u64> d_hi[2], d_selhi, d_marked, d_prank;
    HIPC(h, d_w.alloc((size_t)mm.M));
    HIPC(h, d_w.upload(a->view_weights, (size_t)mm.M, s));
    HIPC(h, d_theta.alloc((size_t)BE * K));
    HIPC(h, d_psi.alloc((size_t)BQ * K));
    HIPC(h, d_S.alloc((size_t)BQ * BE));
    HIPC(h, d_marked.alloc(1));
    HIPC(h, d_marked.fill(0, s));
    if (item_form) {
        const int64_t total = a->q_off[a->nq];
        HIPC(h, d_qoff.alloc((size_t)a->nq + 1));
        HIPC(h, d_qoff.upload(a->q_off, (size_t)a->nq + 1, s));
        HIPC(h, d_qitems.alloc((size_t)total));
        if (total) HIPC(h, d_qitems.upload(a->q_items, (size_t)total, s));
        if (a->q_weights) {
            HIPC(h, d_qw.alloc((size_t)total));
            if (total) HIPC(h, d_qw.upload(a->q_weights, (size_t)total, s));
        }
        if (rk) HIPC(h, d_qlist.alloc((size_t)BQ));
        if (excl) HIPC(h, d_invoff.alloc((size_t)V + 1));
    }
    if (pr) {
        for (int i = 0; i < 2; i++) {
            HIPC(h, d_hi[i].alloc((size_t)BQ * n_cap));
            HIPC(h, d_lo[i].alloc((size_t)BQ * n_cap));
            HIPC(h, d_cnt[i].alloc((size_t)BQ));
        }
        HIPC(h, d_selhi.alloc((size_t)BQ * sel_pitch));
        HIPC(h, d_sello.alloc((size_t)BQ * sel_pitch));
    } else {
        // the pairs by (block of queries, entity): a block's pairs of one block of entities lie together
        order.resize((size_t)rk->n);
        std::vector<int64_t> blk((size_t)rk->n);
        for (int64_t i = 0; i < rk->n; i++) {
            order[(size_t)i] = i;
            blk[(size_t)i] = (std::lower_bound(qsel.begin(), qsel.end(), rk->query[i]) - qsel.begin()) / BQ;
        }
        std::stable_sort(order.begin(), order.end(), [&](int64_t l, int64_t r) {
            return blk[(size_t)l] != blk[(size_t)r] ? blk[(size_t)l] < blk[(size_t)r] : rk->entity[l] < rk->entity[r]; });
    }
    StreamTimer timer;
    HIPC(h, timer.create());
    HIPC(h, timer.start(s));

    std::vector<double> h_psi, c_pscore;
    std::vector<int64_t> h_invoff;
    std::vector<int32_t> h_invq, h_prow, c_cnt;
    std::vector<uint32_t> h_pent, c_lo;
    std::vector<u64> c_hi, c_prank;
    int64_t pcur = 0;                                          // rank: the next pair of `order`

    auto launch_theta = [&](int64_t e0, int64_t ne) { return mvhdp_launch_doc_topic_prop(mm, carry, d_w, a->c0 + e0, a->c0 + e0 + ne, d_theta, s); };

    for (int64_t qb0 = 0; qb0 < nqs; qb0 += BQ) {
        const int64_t nqb = std::min(BQ, nqs - qb0);
        auto query_of = [&](int64_t r) { return rk ? qsel[(size_t)(qb0 + r)] : qb0 + r; };
        // ---- the block's psi rows ----
        if (item_form) {
            if (rk) HIPC(h, d_qlist.upload(qsel.data() + qb0, (size_t)nqb, s));
            LAUNCH(h, xe_psi_kernel, dim3((unsigned)((nqb * K + 255) / 256)), dim3(256), 0, s, d_rows, d_nk, mm.inactive, K, nqb, rk ? d_qlist.get() : nullptr, qb0,
                   d_qoff, d_qitems, a->q_weights ? d_qw.get() : nullptr, mm.beta[m], mm.beta_sum[m], d_psi);
        } else if (rk) {
            h_psi.resize((size_t)nqb * K);
            for (int64_t r = 0; r < nqb; r++) memcpy(h_psi.data() + (size_t)r * K, a->psi + query_of(r) * K, (size_t)K * sizeof(double));
            HIPC(h, d_psi.upload(h_psi.data(), (size_t)nqb * K, s));
        } else
            HIPC(h, d_psi.upload(a->psi + qb0 * K, (size_t)nqb * K, s));
        // ---- type -> the block's query rows that hold it ----
        if (excl) {
            h_invoff.assign((size_t)V + 1, 0);
            for (int64_t r = 0; r < nqb; r++) {
                const int64_t q = query_of(r);
                for (int64_t i = a->q_off[q]; i < a->q_off[q + 1]; i++) h_invoff[(size_t)a->q_items[i] + 1]++;
            }
            for (int64_t w = 0; w < V; w++) h_invoff[(size_t)w + 1] += h_invoff[(size_t)w];
            h_invq.resize((size_t)h_invoff[(size_t)V]);
            std::vector<int64_t> fill(h_invoff.begin(), h_invoff.end() - 1);
            for (int64_t r = 0; r < nqb; r++) {
                const int64_t q = query_of(r);
                for (int64_t i = a->q_off[q]; i < a->q_off[q + 1]; i++) h_invq[(size_t)fill[(size_t)a->q_items[i]]++] = (int32_t)r;
            }
            HIPC(h, d_invoff.upload(h_invoff.data(), (size_t)V + 1, s));
            HIPC(h, d_invq.alloc(h_invq.size()));
            if (!h_invq.empty()) HIPC(h, d_invq.upload(h_invq.data(), h_invq.size(), s));
        }
        auto launch_scores = [&](int64_t e0, int64_t ne) -> int {      // the block of scores [nqb][ne], excluded cells marked
            ScoreArgs ka{};
            ka.theta = d_psi; ka.row_list = nullptr; ka.row0 = 0; ka.phi = d_theta; ka.S = d_S; ka.ldS = ne; ka.col0 = 0;
            ka.n_rows = (int32_t)nqb; ka.n_types = (int32_t)ne; ka.K = K; ka.tiles_w = (int32_t)((ne + XV_BW - 1) / XV_BW);
            const int64_t tiles = ((nqb + XV_BE - 1) / XV_BE) * ka.tiles_w;
            LAUNCH(h, xview_score_kernel, dim3((unsigned)tiles), dim3(256), 0, s, ka);
            if (excl && !h_invq.empty())
                LAUNCH(h, xe_mark_kernel, dim3(wave_blocks(ne, h->num_cus)), dim3(256), 0, s, reinterpret_cast<u64*>(d_S.get()), ne, ne, a->c0 + e0, V, mm.doc_off[m], mm.tok[m],
                       d_invoff, d_invq, d_marked);
            st.cells += nqb * ne;
            st.blocks++;
            return MVHDP_OK;
        };

        if (pr) {
            int flip = 0;
            HIPC(h, d_cnt[0].fill(0, s));
            for (int64_t e0 = 0; e0 < C; e0 += BE, flip ^= 1) {
                const int64_t ne = std::min(BE, C - e0);
                HIPC(h, launch_theta(e0, ne));
                rc = launch_scores(e0, ne); if (rc) return rc;
                PickArgs pa{};
                pa.S = reinterpret_cast<const u64*>(d_S.get()); pa.ld = ne; pa.nrows = (int)nqb; pa.ne = (int)ne; pa.e0 = (uint32_t)e0; pa.n_cap = n_cap;
                pa.in_hi = d_hi[flip]; pa.in_lo = d_lo[flip]; pa.in_cnt = d_cnt[flip];
                pa.out_hi = d_hi[flip ^ 1]; pa.out_lo = d_lo[flip ^ 1]; pa.out_cnt = d_cnt[flip ^ 1];
                pa.sel_hi = d_selhi; pa.sel_lo = d_sello; pa.sel_pitch = sel_pitch;
                if (ne <= XE_LDS_ENTITIES) LAUNCH(h, xe_pick_kernel<true>, dim3(row_blocks(nqb, h->num_cus)), dim3(64), (size_t)ne * sizeof(u64), s, pa);
                else LAUNCH(h, xe_pick_kernel<false>, dim3(row_blocks(nqb, h->num_cus)), dim3(64), 0, s, pa);
            }
            const size_t cells = (size_t)nqb * n_cap;
            c_hi.resize(cells); c_lo.resize(cells); c_cnt.resize((size_t)nqb);
            HIPC(h, d_hi[flip].download(c_hi.data(), cells, s));
            HIPC(h, d_lo[flip].download(c_lo.data(), cells, s));
            HIPC(h, d_cnt[flip].download(c_cnt.data(), (size_t)nqb, s));
            HIPC(h, hipStreamSynchronize(s));
            for (int64_t r = 0; r < nqb; r++) {                 // the slots beyond the count keep id -1 and score 0.0
                const int c = c_cnt[(size_t)r];
                pr->counts[(size_t)(qb0 + r)] = c;
                for (int i = 0; i < c; i++) {
                    const u64 bits = f64_key_bits(c_hi[(size_t)r * n_cap + i]);
                    double v; memcpy(&v, &bits, sizeof v);
                    pr->ids[(size_t)(qb0 + r) * pr->n + i] = a->c0 + (int64_t)(uint32_t)~c_lo[(size_t)r * n_cap + i];
                    pr->scores[(size_t)(qb0 + r) * pr->n + i] = v;
                }
            }
        } else {
            // the block's pairs, by entity
            int64_t pend = pcur;
            h_prow.clear(); h_pent.clear();
            while (pend < rk->n) {
                const int64_t i = order[(size_t)pend];
                const int64_t at = std::lower_bound(qsel.begin(), qsel.end(), rk->query[i]) - qsel.begin();
                if (at >= qb0 + nqb) break;
                h_prow.push_back((int32_t)(at - qb0)); h_pent.push_back((uint32_t)(rk->entity[i] - a->c0));
                pend++;
            }
            const int64_t np = pend - pcur;
            HIPC(h, d_prow.alloc((size_t)np));
            HIPC(h, d_pent.alloc((size_t)np));
            HIPC(h, d_pscore.alloc((size_t)np));
            HIPC(h, d_prank.alloc((size_t)np));
            HIPC(h, d_prow.upload(h_prow.data(), (size_t)np, s));
            HIPC(h, d_pent.upload(h_pent.data(), (size_t)np, s));
            HIPC(h, d_prank.fill(0, s));
            // ---- first the scores of the pairs: every block of entities needs them to count ----
            const bool one_block = C <= BE;
            int64_t at = 0;
            for (int64_t e0 = 0; e0 < C && at < np; e0 += BE) {
                const int64_t ne = std::min(BE, C - e0);
                int64_t to = at;
                while (to < np && (int64_t)h_pent[(size_t)to] < e0 + ne) to++;
                if (to == at) continue;
                HIPC(h, launch_theta(e0, ne));
                LAUNCH(h, xe_pair_score_kernel, dim3((unsigned)((to - at + 255) / 256)), dim3(256), 0, s, d_theta, d_psi, K, to - at, d_prow + at, d_pent + at, (uint32_t)e0,
                       d_pscore + at);
                at = to;
            }
            // ---- then block by block of entities: scores, marks, counts ----
            for (int64_t e0 = 0; e0 < C; e0 += BE) {
                const int64_t ne = std::min(BE, C - e0);
                if (!one_block) HIPC(h, launch_theta(e0, ne));
                rc = launch_scores(e0, ne); if (rc) return rc;
                LAUNCH(h, xe_rank_kernel, dim3(wave_blocks(np, h->num_cus)), dim3(256), 0, s, reinterpret_cast<const u64*>(d_S.get()), ne, (int)ne, (uint32_t)e0, np, d_prow, d_pent,
                       reinterpret_cast<const u64*>(d_pscore.get()), d_prank);
            }
            c_pscore.resize((size_t)np); c_prank.resize((size_t)np);
            HIPC(h, d_pscore.download(c_pscore.data(), (size_t)np, s));
            HIPC(h, d_prank.download(c_prank.data(), (size_t)np, s));
            HIPC(h, hipStreamSynchronize(s));
            for (int64_t i = 0; i < np; i++) {
                const size_t to = (size_t)order[(size_t)(pcur + i)];
                rk->score[to] = c_pscore[(size_t)i]; rk->rank[to] = (int64_t)c_prank[(size_t)i];
            }
            pcur = pend;
        }
    }
    u64 marked = 0;
    HIPC(h, timer.stop(s));
    HIPC(h, d_marked.download(&marked, 1, s));
    HIPC(h, hipStreamSynchronize(s));
    HIPC(h, timer.elapsed_ms(&st.kernel_ms));
    st.excluded = (int64_t)marked;
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_predict_entities(mvhdp_handle h, const mvhdp_entities_args* a, int32_t n, int64_t* ids, double* scores, int32_t* counts, mvhdp_entities_stats* stats)
{
    CHECK_H(h);
    int rc = check_args(h, a, "predict_entities"); if (rc) return rc;
    if (n < 1 || n > XE_MAX_N) FAIL(h, MVHDP_ERR_INVALID_ARG, "predict_entities: n outside 1..1024");
    if (!ids || !scores || !counts) FAIL(h, MVHDP_ERR_INVALID_ARG, "predict_entities: a null output");
    mvhdp_entities_stats st{};
    if (a->nq == 0) { if (stats) *stats = st; return MVHDP_OK; }
    EntPredict pr;
    pr.n = n;
    pr.ids.assign((size_t)a->nq * n, -1); pr.scores.assign((size_t)a->nq * n, 0.0); pr.counts.assign((size_t)a->nq, 0);
    if (a->c1 > a->c0) { rc = entities_run(h, a, &pr, nullptr, st); if (rc) return rc; }
    memcpy(ids, pr.ids.data(), pr.ids.size() * sizeof(int64_t));
    memcpy(scores, pr.scores.data(), pr.scores.size() * sizeof(double));
    memcpy(counts, pr.counts.data(), pr.counts.size() * sizeof(int32_t));
    if (stats) *stats = st;
    return MVHDP_OK;
}

extern "C" int mvhdp_rank_entities(mvhdp_handle h, const mvhdp_entities_args* a, int64_t n_pairs, const int64_t* query, const int64_t* entity, double* score, int64_t* rank)
{
    CHECK_H(h);
    int rc = check_args(h, a, "rank_entities"); if (rc) return rc;
    if (n_pairs < 0 || !score || !rank || (n_pairs > 0 && (!query || !entity))) FAIL(h, MVHDP_ERR_INVALID_ARG, "rank_entities: negative n_pairs or a null array");
    for (int64_t i = 0; i < n_pairs; i++) {
        if (query[i] < 0 || query[i] >= a->nq) FAIL(h, MVHDP_ERR_INVALID_ARG, "rank_entities: a query index outside [0, nq)");
        if (entity[i] < a->c0 || entity[i] >= a->c1) FAIL(h, MVHDP_ERR_INVALID_ARG, "rank_entities: an entity outside [c0, c1)");
    }
    if (n_pairs == 0) return MVHDP_OK;
    EntRank rk;
    rk.n = n_pairs; rk.query = query; rk.entity = entity;
    rk.score.assign((size_t)n_pairs, 0.0); rk.rank.assign((size_t)n_pairs, 0);
    mvhdp_entities_stats st{};
    rc = entities_run(h, a, nullptr, &rk, st); if (rc) return rc;
    memcpy(score, rk.score.data(), (size_t)n_pairs * sizeof(double));
    memcpy(rank, rk.rank.data(), (size_t)n_pairs * sizeof(int64_t));
    return MVHDP_OK;
}
