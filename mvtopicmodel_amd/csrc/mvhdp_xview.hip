// mvhdp_xview.hip — cross-view prediction: rank the types of one view for an entity by score(d, w) = sum_k theta_d[k] * phi[w][k]
// (include/mvhdp.h has the contract: the chain, the order, the excluded set; tests/native/xview_ref.c restates it on the host).
//   xview_phi_kernel, xview_score_kernel
//                         the phi table and the tiled fp64 chain: mvhdp_xview.h, shared with mvhdp_xview_entities.hip.
//   xview_pair_score_kernel, xview_mark_kernel, xview_select_kernel, xview_order_kernel, xview_rank_kernel
//                         the selection behind it, on the block of scores [rows][V]: the queried scores are read; the entries of the
//                         excluded types are overwritten with a marker whose key is 0; one wave per row finds the key of the n-th entry
//                         by a bitwise descent on an order-preserving 64-bit key (the row's keys in LDS while they fit 64 KiB, every
//                         lane counting its own share of a pass), compacts the row's first n entries (ascending type id) and a
//                         second kernel places each by the number that precede it; one wave per pair counts the entries that
//                         precede the queried one (wave_rank_count of mvhdp_select.h).  Integers and exact fp64 values only.
//                         (The select / order pair is not wave_first_n of mvhdp_select.h, which the other top-n picks call: as one
//                         pick kernel on it the LDS form measured 18 % slower, profiles/select_refactor.md.)
// Work is cut on the host: theta in ranges of entities, scores in blocks of rows, phi in stripes of types, each within XVIEW_BLOCK_BYTES.
// Everything runs on the handle's stream; the shared argument checks, the prologue and wave_blocks are mvhdp_side.h's.
#include "mvhdp_side.h"
#include "mvhdp_select.h"
#include "mvhdp_xview.h"

namespace {

constexpr size_t XVIEW_BLOCK_BYTES = (size_t)256 << 20;        // the block of scores, the phi stripe and the theta range: each at most this
constexpr size_t XV_SELECT_LDS_BYTES = 64 << 10;                  // a row of keys up to this size is selected from LDS (V_m <= 8192)

// one thread per pair: the score as the block holds it, before any entry is marked
__global__ __launch_bounds__(256) void xview_pair_score_kernel(const double* __restrict__ S, int64_t V, int64_t n_pairs, const int32_t* __restrict__ pair_row,
                                                               const int32_t* __restrict__ pair_item, double* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_pairs) out[p] = S[(int64_t)pair_row[p] * V + pair_item[p]];
}

// one wave per row: the types < V of the entity's view-m span are excluded
__global__ __launch_bounds__(256) void xview_mark_kernel(u64* __restrict__ S, int64_t V, int64_t n_rows, const int64_t* __restrict__ row_entity,
                                                         const int64_t* __restrict__ doc_off, const int32_t* __restrict__ tok)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < n_rows; r += nwaves) {
        const int64_t d = row_entity[r], b = doc_off[d], e = doc_off[d + 1];
        for (int64_t i = b + lane; i < e; i += 64) {
            const int32_t w = tok[i];
            if (w >= 0 && (int64_t)w < V) S[r * V + w] = XV_EXCLUDED;
        }
    }
}

// one wave per row: counts[r] = min(n, entries that are not excluded); the first counts[r] entries of the order (key descending, equal
// keys by ascending type) go to sel_key / sel_id [r][n_cap] in ascending type id.  The descent reads the row once per bit that the keys
// do not share, some fifty times: IN_LDS (a row of keys fits XV_SELECT_LDS_BYTES) a one-wave block keeps the keys in LDS and goes to
// memory once; otherwise the passes read the block of scores where it lies (the wave's row stays in L2).
template <bool IN_LDS>
__global__ __launch_bounds__(IN_LDS ? 64 : 256) void xview_select_kernel(const u64* __restrict__ S, int64_t V, int64_t n_rows, int32_t n_cap, int32_t* __restrict__ counts,
                                                                         u64* __restrict__ sel_key, int32_t* __restrict__ sel_id)
{
    extern __shared__ u64 s_keys[];                            // IN_LDS: [V]
    const int lane = threadIdx.x & 63;
    const u64 lt_mask = lanes_below(lane);
    const int64_t wave = IN_LDS ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = IN_LDS ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < n_rows; r += nwaves) {
        const u64* __restrict__ row = S + r * V;
        auto key_at = [&](int64_t w) -> u64 { return w < V ? (IN_LDS ? s_keys[w] : f64_bits_key(row[w])) : 0; };
        // how many keys of the row pass the test: every lane counts its own (w = lane, lane + 64, ..), the 64 counts are added at the end
        auto count_keys = [&](auto&& test) -> int64_t {
            int c = 0;
#pragma unroll 8
            for (int64_t w = lane; w < V; w += 64) c += test(IN_LDS ? s_keys[w] : f64_bits_key(row[w])) ? 1 : 0;
            return (int64_t)wave_sum(c);
        };
        if (IN_LDS) {
            __syncthreads();                                   // (one wave: the reads of the row before are done)
            for (int64_t w = lane; w < V; w += 64) s_keys[w] = f64_bits_key(row[w]);
            __syncthreads();
        }
        int nv = 0;
        u64 all_and = ~0ull, all_or = 0;
#pragma unroll 8
        for (int64_t w = lane; w < V; w += 64) {
            const u64 key = IN_LDS ? s_keys[w] : f64_bits_key(row[w]);
            if (key != 0) { nv++; all_and &= key; all_or |= key; }
        }
        for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); all_and &= __shfl_xor(all_and, o, 64); all_or |= __shfl_xor(all_or, o, 64); }   // one butterfly for the three
        const int64_t valid = nv;
        const int64_t n_eff = valid < (int64_t)n_cap ? valid : (int64_t)n_cap;
        if (lane == 0) counts[r] = (int32_t)n_eff;
        if (n_eff == 0) continue;
        // the largest T that at least n_eff keys reach; the bits every key shares are settled
        const u64 diff = all_and ^ all_or;
        u64 T = all_and;
        if (diff) {
            const int hb = 63 - __builtin_clzll(diff);
            T = key_descent(hb == 63 ? 0 : all_and & ~((2ull << hb) - 1), hb, [&](u64 trial) { return count_keys([&](u64 key) { return key >= trial; }) >= n_eff; });
        }
        const int64_t need_eq = n_eff - count_keys([&](u64 key) { return key > T; });                // >= 1: fewer than n_eff keys lie above T
        int64_t taken_eq = 0, at = 0;
        u64* __restrict__ ok = sel_key + r * n_cap;
        int32_t* __restrict__ oi = sel_id + r * n_cap;
        for (int64_t base = 0; base < V; base += 64) {
            const int64_t w = base + lane;
            const u64 key = key_at(w);
            const u64 eq_b = ballot(key == T && key != 0);
            const bool sel = key > T || (key == T && key != 0 && taken_eq + (int64_t)__builtin_popcountll(eq_b & lt_mask) < need_eq);
            const u64 sel_b = ballot(sel);
            if (sel) {
                const int64_t pos = at + (int64_t)__builtin_popcountll(sel_b & lt_mask);
                ok[pos] = key; oi[pos] = (int32_t)w;
            }
            taken_eq += (int64_t)__builtin_popcountll(eq_b);
            at += (int64_t)__builtin_popcountll(sel_b);
        }
    }
}

// one wave per row: entry i of the compacted list goes to the place given by the number of entries that precede it (the list is in
// ascending type id, so among equal keys the earlier entry precedes)
__global__ __launch_bounds__(256) void xview_order_kernel(const double* __restrict__ S, int64_t V, int64_t n_rows, int32_t n_cap, const int32_t* __restrict__ counts,
                                                          const u64* __restrict__ sel_key, const int32_t* __restrict__ sel_id, int32_t* __restrict__ items,
                                                          double* __restrict__ scores)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < n_rows; r += nwaves) {
        const int n = counts[r];
        const u64* __restrict__ sk = sel_key + r * n_cap;
        const int32_t* __restrict__ si = sel_id + r * n_cap;
        for (int i = lane; i < n_cap; i += 64) {
            if (i < n) {
                const u64 ki = sk[i];
                int pos = 0;
                for (int j = 0; j < n; j++) { const u64 kj = sk[j]; pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0; }
                const int32_t w = si[i];
                items[r * n_cap + pos] = w;
                scores[r * n_cap + pos] = S[r * V + w];
            } else {
                items[r * n_cap + i] = -1;
                scores[r * n_cap + i] = 0.0;
            }
        }
    }
}

// one wave per pair: the entries of the row, the queried type apart, that are not excluded and precede it
__global__ __launch_bounds__(256) void xview_rank_kernel(const u64* __restrict__ S, int64_t V, int64_t n_pairs, const int32_t* __restrict__ pair_row,
                                                         const int32_t* __restrict__ pair_item, const u64* __restrict__ pair_score, int32_t* __restrict__ rank)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t p = wave; p < n_pairs; p += nwaves) {
        const int c = wave_rank_count(S + (int64_t)pair_row[p] * V, (int)V, 0u, f64_bits_key(pair_score[p]), (uint32_t)pair_item[p], lane);
        if (lane == 0) rank[p] = c;
    }
}

// MVHDP_XVIEW_BLOCK_BYTES (tests: forces the borders between blocks, stripes and ranges at small sizes)
size_t block_bytes()
{
    if (const char* e = getenv("MVHDP_XVIEW_BLOCK_BYTES")) { const long long v = atoll(e); if (v >= 8) return (size_t)v; }
    return XVIEW_BLOCK_BYTES;
}

// MVHDP_XVIEW_SELECT_LDS_BYTES (measurements: 0 selects every row from the block of scores): at most XV_SELECT_LDS_BYTES
size_t select_lds_bytes()
{
    if (const char* e = getenv("MVHDP_XVIEW_SELECT_LDS_BYTES")) { const long long v = atoll(e); if (v >= 0 && (size_t)v <= XV_SELECT_LDS_BYTES) return (size_t)v; }
    return XV_SELECT_LDS_BYTES;
}

struct PairWork {                                              // mvhdp_score_items: the pairs sorted by entity
    int64_t n = 0;
    const int64_t* entity = nullptr;
    const int32_t* item = nullptr;
    std::vector<int64_t> order;                                // pair indices, by (entity, index)
    double* score = nullptr;
    int32_t* rank = nullptr;
    std::vector<double> h_score;
    std::vector<int32_t> h_rank;
};

struct PredictWork {
    int32_t n = 0;
    std::vector<int32_t> items, counts;
    std::vector<double> scores;
};

// the arguments both calls share; every check comes before the first output is touched
int check_common(mvhdp_ctx* h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, const char* who)
{
    MvModel& mm = h->mm;
    const std::string w(who);
    if (!a) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": null arguments");
    if (a->m < 0 || a->m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": bad view");
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, w + " before set_hyper");
    rc = require_current_counts(h, w); if (rc) return rc;
    if (d0 < 0 || d1 > mm.D || d0 > d1) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": bad entity range");
    if (a->theta) {
        if (const char* r = check_nonneg_finite(a->theta, (d1 - d0) * mm.K)) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": a theta entry " + r);
    } else {
        if (!a->view_weights) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": neither view_weights nor theta");
        if (const char* r = check_view_weights(a->view_weights, mm.M)) FAIL(h, MVHDP_ERR_INVALID_ARG, w + ": " + r);
    }
    return MVHDP_OK;
}

// The work of both calls.  pw: score the pairs; else pr: the first pr->n types of every entity of [d0, d1).
int xview_run(mvhdp_ctx* h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, PairWork* pw, PredictWork* pr)
{
    MvModel& mm = h->mm;
    const int K = mm.K, m = a->m;
    const int64_t V = mm.V[m];
    const bool excl = a->exclude_present != 0;
    const size_t bb = block_bytes();
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    DocTopicCarry carry{};
    DevArray<double> d_w;
    if (!a->theta) {
        int rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
        HIPC(h, d_w.alloc((size_t)mm.M));
        HIPC(h, d_w.upload(a->view_weights, (size_t)mm.M, s));
    }
    const int32_t* d_rows = mm.counts + mm.rowbase[m] * K;
    const int32_t* d_nk = mm.counts + mm.rowbase[mm.M] * K + (int64_t)m * K;

    // the sizes of the cuts: entities per theta range, rows per block of scores, types per phi stripe
    const int64_t per_k = std::max<int64_t>(1, (int64_t)(bb / ((size_t)K * sizeof(double))));
    const int64_t range_len = std::min<int64_t>(per_k, (int64_t)1 << 30);
    const int64_t block_rows = std::max<int64_t>(1, std::min<int64_t>((int64_t)(bb / ((size_t)V * sizeof(double))), (int64_t)1 << 24));
    const int64_t stripe = std::min<int64_t>(V, per_k);
    const bool one_stripe = stripe >= V;
    DevArray<double> d_phi;
    HIPC(h, d_phi.alloc((size_t)stripe * K));
    auto launch_phi = [&](int64_t v0, int64_t nv) {
        const int64_t cells = nv * K;
        hipLaunchKernelGGL(xview_phi_kernel, dim3((unsigned)std::min<int64_t>((cells + 255) / 256, (int64_t)h->num_cus * 16)), dim3(256), 0, s,
                           d_rows + v0 * K, d_nk, mm.inactive, K, cells, mm.beta[m], mm.beta_sum[m], d_phi.get());
        return hipGetLastError();
    };
    if (one_stripe) HIPC(h, launch_phi(0, V));

    const int32_t n_cap = pr ? (int32_t)std::min<int64_t>(pr->n, V) : 0;
    DevArray<double> d_theta, d_S, d_scores, d_pscore;          // d_S and d_pscore are also read as u64 keys (the mark, rank and select kernels)
    DevArray<int64_t> d_ent;
    DevArray<int32_t> d_list, d_counts, d_seli, d_items, d_prow, d_pitem, d_prank;
    DevArray<u64> d_selk;
    std::vector<int64_t> h_ent;
    std::vector<int32_t> h_list, h_prow, h_pitem, c_items, c_counts, c_rank;
    std::vector<double> c_scores, c_pscore;
    int64_t pcur = 0;                                          // score_items: the next pair of pw->order
    const int64_t max_range = std::min(range_len, d1 - d0), max_nr = std::min(block_rows, pw ? std::min(pw->n, d1 - d0) : d1 - d0);
    HIPC(h, d_theta.alloc((size_t)max_range * K));
    HIPC(h, d_S.alloc((size_t)max_nr * V));
    if (excl) HIPC(h, d_ent.alloc((size_t)max_nr));
    if (pw) HIPC(h, d_list.alloc((size_t)max_nr));
    else {
        HIPC(h, d_counts.alloc((size_t)max_nr));
        HIPC(h, d_selk.alloc((size_t)max_nr * n_cap));
        HIPC(h, d_seli.alloc((size_t)max_nr * n_cap));
        HIPC(h, d_items.alloc((size_t)max_nr * n_cap));
        HIPC(h, d_scores.alloc((size_t)max_nr * n_cap));
    }

    for (int64_t c0 = d0; c0 < d1; c0 += range_len) {
        const int64_t c1 = std::min(d1, c0 + range_len);
        // the rows of this range: every entity (predict), or those that have pairs, each once, with its pairs behind it
        int64_t n_rows_range = c1 - c0, pend = pcur;
        if (pw) {
            h_list.clear();
            while (pend < pw->n && pw->entity[pw->order[(size_t)pend]] < c1) {
                const int64_t e = pw->entity[pw->order[(size_t)pend]];
                if (h_list.empty() || h_list.back() != (int32_t)(e - c0)) h_list.push_back((int32_t)(e - c0));
                pend++;
            }
            n_rows_range = (int64_t)h_list.size();
            if (n_rows_range == 0) continue;
        }
        if (a->theta) HIPC(h, d_theta.upload(a->theta + (c0 - d0) * K, (size_t)(c1 - c0) * K, s));
        else HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, d_w, c0, c1, d_theta, s));

        for (int64_t r0 = 0; r0 < n_rows_range; r0 += block_rows) {
            const int64_t nr = std::min(block_rows, n_rows_range - r0);
            h_ent.resize((size_t)nr);
            for (int64_t r = 0; r < nr; r++) h_ent[(size_t)r] = c0 + (pw ? (int64_t)h_list[(size_t)(r0 + r)] : r0 + r);
            if (pw)
                HIPC(h, d_list.upload(h_list.data() + r0, (size_t)nr, s));
            // ---- scores: stripe by stripe of types ----
            ScoreArgs ka{};
            ka.theta = d_theta; ka.row_list = pw ? d_list.get() : nullptr; ka.row0 = r0;
            ka.phi = d_phi; ka.S = d_S; ka.ldS = V; ka.n_rows = (int32_t)nr; ka.K = K;
            for (int64_t v0 = 0; v0 < V; v0 += stripe) {
                const int64_t nv = std::min(stripe, V - v0);
                if (!one_stripe) HIPC(h, launch_phi(v0, nv));
                ka.col0 = v0; ka.n_types = (int32_t)nv; ka.tiles_w = (int32_t)((nv + XV_BW - 1) / XV_BW);
                const int64_t tiles = ((nr + XV_BE - 1) / XV_BE) * ka.tiles_w;
                LAUNCH(h, xview_score_kernel, dim3((unsigned)tiles), dim3(256), 0, s, ka);
            }
            // ---- the pairs of these rows: their scores before anything is marked ----
            int64_t np = 0;
            if (pw) {
                h_prow.clear(); h_pitem.clear();
                int64_t q = pcur;
                for (int64_t r = 0; r < nr; r++)
                    while (q < pend && pw->entity[pw->order[(size_t)q]] == h_ent[(size_t)r]) {
                        h_prow.push_back((int32_t)r); h_pitem.push_back(pw->item[pw->order[(size_t)q]]); q++;
                    }
                np = q - pcur;
                HIPC(h, d_prow.alloc((size_t)np));
                HIPC(h, d_pitem.alloc((size_t)np));
                HIPC(h, d_pscore.alloc((size_t)np));
                HIPC(h, d_prank.alloc((size_t)np));
                HIPC(h, d_prow.upload(h_prow.data(), (size_t)np, s));
                HIPC(h, d_pitem.upload(h_pitem.data(), (size_t)np, s));
                LAUNCH(h, xview_pair_score_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, d_S, V, np, d_prow, d_pitem, d_pscore);
            }
            if (excl) {
                HIPC(h, d_ent.upload(h_ent.data(), (size_t)nr, s));
                LAUNCH(h, xview_mark_kernel, dim3(wave_blocks(nr, h->num_cus)), dim3(256), 0, s, reinterpret_cast<u64*>(d_S.get()), V, nr, d_ent, mm.doc_off[m], mm.tok[m]);
            }
            if (pw) {
                LAUNCH(h, xview_rank_kernel, dim3(wave_blocks(np, h->num_cus)), dim3(256), 0, s, reinterpret_cast<u64*>(d_S.get()), V, np, d_prow, d_pitem,
                       reinterpret_cast<u64*>(d_pscore.get()), d_prank);
                c_pscore.resize((size_t)np); c_rank.resize((size_t)np);
                HIPC(h, d_pscore.download(c_pscore.data(), (size_t)np, s));
                HIPC(h, d_prank.download(c_rank.data(), (size_t)np, s));
                HIPC(h, hipStreamSynchronize(s));
                for (int64_t i = 0; i < np; i++) {
                    const size_t at = (size_t)pw->order[(size_t)(pcur + i)];
                    pw->h_score[at] = c_pscore[(size_t)i]; pw->h_rank[at] = c_rank[(size_t)i];
                }
                pcur += np;
            } else {
                const size_t cells = (size_t)nr * n_cap;
                if ((size_t)V * sizeof(u64) <= select_lds_bytes())
                    LAUNCH(h, xview_select_kernel<true>, dim3((unsigned)std::min<int64_t>(nr, (int64_t)h->num_cus * 32)), dim3(64), (size_t)V * sizeof(u64), s,
                           reinterpret_cast<u64*>(d_S.get()), V, nr, n_cap, d_counts, d_selk, d_seli);
                else
                    LAUNCH(h, xview_select_kernel<false>, dim3(wave_blocks(nr, h->num_cus)), dim3(256), 0, s, reinterpret_cast<u64*>(d_S.get()), V, nr, n_cap, d_counts, d_selk, d_seli);
                LAUNCH(h, xview_order_kernel, dim3(wave_blocks(nr, h->num_cus)), dim3(256), 0, s, d_S, V, nr, n_cap, d_counts, d_selk, d_seli, d_items, d_scores);
                c_items.resize(cells); c_scores.resize(cells); c_counts.resize((size_t)nr);
                HIPC(h, d_items.download(c_items.data(), cells, s));
                HIPC(h, d_scores.download(c_scores.data(), cells, s));
                HIPC(h, d_counts.download(c_counts.data(), (size_t)nr, s));
                HIPC(h, hipStreamSynchronize(s));
                for (int64_t r = 0; r < nr; r++) {              // the slots beyond n_cap keep item -1 and score 0.0
                    const size_t to = (size_t)(c0 - d0 + r0 + r) * (size_t)pr->n, from = (size_t)r * n_cap;
                    memcpy(pr->items.data() + to, c_items.data() + from, (size_t)n_cap * sizeof(int32_t));
                    memcpy(pr->scores.data() + to, c_scores.data() + from, (size_t)n_cap * sizeof(double));
                    pr->counts[(size_t)(c0 - d0 + r0 + r)] = c_counts[(size_t)r];
                }
            }
        }
        pcur = pw ? pend : pcur;
    }
    HIPC(h, hipStreamSynchronize(s));
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_predict_items(mvhdp_handle h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, int32_t n, int32_t* items, double* scores, int32_t* counts)
{
    CHECK_H(h);
    int rc = check_common(h, a, d0, d1, "predict_items"); if (rc) return rc;
    if (n < 1 || !items || !scores || !counts) FAIL(h, MVHDP_ERR_INVALID_ARG, "predict_items: n < 1 or a null output");
    if (d0 == d1) return MVHDP_OK;
    const size_t D = (size_t)(d1 - d0);
    PredictWork pr;
    pr.n = n;
    pr.items.assign(D * (size_t)n, -1); pr.scores.assign(D * (size_t)n, 0.0); pr.counts.assign(D, 0);
    rc = xview_run(h, a, d0, d1, nullptr, &pr); if (rc) return rc;
    memcpy(items, pr.items.data(), pr.items.size() * sizeof(int32_t));
    memcpy(scores, pr.scores.data(), pr.scores.size() * sizeof(double));
    memcpy(counts, pr.counts.data(), pr.counts.size() * sizeof(int32_t));
    return MVHDP_OK;
}

extern "C" int mvhdp_score_items(mvhdp_handle h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, int64_t n_pairs, const int64_t* entity, const int32_t* item,
                                 double* score, int32_t* rank)
{
    CHECK_H(h);
    int rc = check_common(h, a, d0, d1, "score_items"); if (rc) return rc;
    if (n_pairs < 0 || !score || !rank || (n_pairs > 0 && (!entity || !item))) FAIL(h, MVHDP_ERR_INVALID_ARG, "score_items: negative n_pairs or a null array");
    const int32_t V = h->mm.V[a->m];
    for (int64_t i = 0; i < n_pairs; i++) {
        if (entity[i] < d0 || entity[i] >= d1) FAIL(h, MVHDP_ERR_INVALID_ARG, "score_items: an entity outside [d0, d1)");
        if (item[i] < 0 || item[i] >= V) FAIL(h, MVHDP_ERR_INVALID_ARG, "score_items: an item outside the view's types");
    }
    if (d0 == d1 || n_pairs == 0) return MVHDP_OK;
    PairWork pw;
    pw.n = n_pairs; pw.entity = entity; pw.item = item;
    pw.order.resize((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; i++) pw.order[(size_t)i] = i;
    std::stable_sort(pw.order.begin(), pw.order.end(), [&](int64_t l, int64_t r) { return entity[l] < entity[r]; });
    pw.h_score.assign((size_t)n_pairs, 0.0); pw.h_rank.assign((size_t)n_pairs, 0);
    rc = xview_run(h, a, d0, d1, &pw, nullptr); if (rc) return rc;
    memcpy(score, pw.h_score.data(), (size_t)n_pairs * sizeof(double));
    memcpy(rank, pw.h_rank.data(), (size_t)n_pairs * sizeof(int32_t));
    return MVHDP_OK;
}
