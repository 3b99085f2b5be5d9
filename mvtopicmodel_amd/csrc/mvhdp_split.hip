// mvhdp_split.hip — mvhdp_split_topic: cut one topic of the trained handle in two with a restricted Gibbs sampler (include/mvhdp.h has the
// contract; tests/native/split_ref.c restates it on the host).  Only the tokens that carry the source topic are touched: they are listed
// once, and every iteration works on the list and on a side table of two columns, never on the full z or the [V][K] rows again.
//   split_scan_kernel<WRITE>  over one view's z with 16-byte loads, every block a contiguous range of tiles of 1024 tokens.  WRITE = false
//                             counts the block's tokens of the source; the host scans the block counts.  WRITE = true lists them in position
//                             order (a block scan per tile): position, type and the initial side byte (the hint, else the coin of
//                             iteration 0; the entity is found by bisection of doc_off).
//   split_csr_kernel          per entity and view the first record at or behind the entity's span (bisection of the record positions):
//                             the CSR of the records by entity; an entity that owns a record is appended to the owner list.
//   split_column_kernel       the source column of the sumV + M count rows into the side table [sumV + M][2] (side a; b = 0).
//   split_apply_kernel        integer atomics on the side table for the records whose side differs between two side arrays (old = nullptr:
//                             from "all a", the fill behind the initial sides); n_k's row and flips are reduced per block.
//   split_sample_kernel       one wave per owner entity and iteration.  The frozen table and the old sides are read, the new sides written
//                             to the other side array: nothing it writes is read by it.  Per view the wave goes through the entity's
//                             records in chunks of 64: every lane forms u (Philox) and both phi of its record, then the chain through
//                             the live e[m][x] is resolved record by record from the wave's LDS slice, the same on every lane.
//   split_finish_kernel       z of the records on side b; split_store_kernel the two columns back into the count rows.
// alpha, the inactive set and the choice of the target are K-sized and stay on the host.
#include "mvhdp_side.h"
#include "mvhdp_wave.h"
#include "mvhdp_select.h"

namespace {

enum { SPLIT_TILE = 1024 };                                    // tokens of a tile: 256 lanes, a 16-byte load each

struct SplitView {
    const int64_t* off;                // [D + 1]
    const int32_t* tok;
    int32_t* z;
    int64_t n, rowbase, rbase;         // tokens; first count row; first record of the view in the record arrays
    int32_t V;
    double beta, beta_sum, A /* gamma * 0.5 alpha[source] */, gas /* gamma * alphaSum */;
};

struct SplitArgs {
    SplitView v[MVHDP_MAXM];
    double P[MVHDP_MAXM * MVHDP_MAXM];
    int64_t D, doc_global0, nrec, nrows /* sumV + M */, sumV;
    int32_t M, K, source, target;
    uint32_t seed_lo, seed_hi;
    const int8_t* hint;                // [sumV]
    int64_t* rec_n;                    // [nrec] position in the view's z
    int32_t* rec_w;                    // [nrec] type
    int64_t* est;                      // [M][D + 1] records of view m in front of entity d's span
    int32_t* owners;                   // [D]
    unsigned int* n_owners;
    int32_t* tab;                      // [sumV + M][2]
};

__device__ __forceinline__ int64_t entity_of(const int64_t* __restrict__ off, int64_t D, int64_t n)
{
    int64_t lo = 0, hi = D;                                    // the last d with off[d] <= n
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= n) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double split_unit(const SplitArgs& a, uint64_t g, uint32_t it, int m, uint32_t pos)
{
    uint32_t x[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), it | ((uint32_t)m << 16), pos, a.seed_lo, a.seed_hi, x);
    return bits_to_unit(x[0], x[1]);
}

// the view of record i: the last one whose records start at or in front of it (no branch: a wave's records may lie in two views)
__device__ __forceinline__ int view_of(const SplitArgs& a, int64_t i)
{
    int m = 0;
#pragma unroll
    for (int j = 1; j < MVHDP_MAXM; j++) m += (j < a.M && i >= a.v[j].rbase) ? 1 : 0;
    return m;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void split_scan_kernel(const SplitArgs a, int m, int64_t tiles_per_block, const int64_t* __restrict__ blk_base,
                                                         int64_t* __restrict__ blk_count, uint8_t* __restrict__ side)
{
    __shared__ int s_w[4];
    __shared__ unsigned long long s_total;
    const SplitView& v = a.v[m];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = v.n, ntiles = (n + SPLIT_TILE - 1) / SPLIT_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block, t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
    int64_t run = WRITE ? blk_base[blockIdx.x] : 0;            // block-uniform
    const int64_t rend = m + 1 < a.M ? a.v[m + 1].rbase : a.nrec;
    int64_t mine = 0;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t i = t * SPLIT_TILE + (int64_t)threadIdx.x * 4;
        int4 q = make_int4(-1, -1, -1, -1);
        if (i + 3 < n) q = *(const int4*)(v.z + i);            // every view's z is an allocation of its own: 16-byte borders
        else {
            if (i < n) q.x = v.z[i];
            if (i + 1 < n) q.y = v.z[i + 1];
            if (i + 2 < n) q.z = v.z[i + 2];
        }
        const int src = a.source;
        const int cnt = (q.x == src) + (q.y == src) + (q.z == src) + (q.w == src);
        if constexpr (!WRITE) { mine += cnt; continue; }
        int incl = cnt;
        for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; w++) { before += w < wave ? s_w[w] : 0; total += s_w[w]; }
        __syncthreads();
        int64_t at = v.rbase + run + before + incl - cnt;
        run += total;
        const int zs[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (zs[j] != src) continue;
            const int64_t pos_n = i + j;
            int32_t w = v.tok[pos_n];
            if ((uint32_t)w >= (uint32_t)v.V) w = -1;          // (no corpus with counts holds one: it has no count row, and none is touched)
            const int hint = w >= 0 ? (int)a.hint[v.rowbase + w] : -1;
            int s = hint;
            if (hint < 0) {
                const int64_t d = entity_of(v.off, a.D, pos_n);
                s = split_unit(a, (uint64_t)(a.doc_global0 + d), 0u, m, (uint32_t)(pos_n - v.off[d])) >= 0.5 ? 1 : 0;
            }
            if (at < rend) { a.rec_n[at] = pos_n; a.rec_w[at] = w; side[at] = (uint8_t)s; }   // (the count pass saw the same z: always)
            at++;
        }
    }
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) s_total = 0;
        __syncthreads();
        if (mine) atomicAdd(&s_total, (unsigned long long)mine);
        __syncthreads();
        if (threadIdx.x == 0) blk_count[blockIdx.x] = (int64_t)s_total;
    }
}

__global__ __launch_bounds__(256) void split_csr_kernel(const SplitArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > a.D) return;
    bool owns = false;
    for (int m = 0; m < a.M; m++) {
        const SplitView& v = a.v[m];
        const int64_t nr = (m + 1 < a.M ? a.v[m + 1].rbase : a.nrec) - v.rbase;
        const int64_t* __restrict__ rn = a.rec_n + v.rbase;
        const int64_t key = v.off[d];
        int64_t lo = 0, hi = nr;                               // the first record with rec_n >= key
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (rn[mid] < key) lo = mid + 1; else hi = mid;
        }
        a.est[(int64_t)m * (a.D + 1) + d] = lo;
        if (d < a.D) owns = owns || (lo < nr && rn[lo] < v.off[d + 1]);
    }
    if (owns) a.owners[atomicAdd(a.n_owners, 1u)] = (int32_t)d;
}

__global__ __launch_bounds__(256) void split_column_kernel(const int32_t* __restrict__ counts, int64_t nrows, int K, int source, int32_t* __restrict__ tab)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    tab[2 * r] = counts[r * K + source];
    tab[2 * r + 1] = 0;
}

__global__ __launch_bounds__(256) void split_store_kernel(int32_t* __restrict__ counts, int64_t nrows, int K, int source, int target, const int32_t* __restrict__ tab)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const int ca = tab[2 * r], cb = tab[2 * r + 1];
    if (counts[r * K + source] != ca) counts[r * K + source] = ca;
    if (cb != 0) counts[r * K + target] = cb;                   // the target's column was all zero
}

// old == nullptr: every record was on side a
__global__ __launch_bounds__(256) void split_apply_kernel(const SplitArgs a, const uint8_t* __restrict__ old, const uint8_t* __restrict__ now, u64* __restrict__ flips)
{
    __shared__ int s_db[MVHDP_MAXM];                           // what side b of view m gains
    __shared__ unsigned int s_flips;
    if (threadIdx.x < MVHDP_MAXM) s_db[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_flips = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nrec) {
        const int o = old ? (int)old[i] : 0, s = (int)now[i];
        if (o != s) {
            const int m = view_of(a, i);
            const int32_t w = a.rec_w[i];
            if (w >= 0) {
                const int64_t r = a.v[m].rowbase + w;
                atomicAdd(&a.tab[2 * r + s], 1);
                atomicSub(&a.tab[2 * r + o], 1);
            }
            atomicAdd(&s_db[m], s ? 1 : -1);
            atomicAdd(&s_flips, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < a.M && s_db[threadIdx.x] != 0) {
        const int64_t r = a.sumV + threadIdx.x;
        atomicAdd(&a.tab[2 * r + 1], s_db[threadIdx.x]);
        atomicSub(&a.tab[2 * r], s_db[threadIdx.x]);
    }
    if (threadIdx.x == 0 && flips && s_flips) atomicAdd(flips, (u64)s_flips);
}

__global__ __launch_bounds__(256) void split_sample_kernel(const SplitArgs a, uint32_t it, int64_t n_owners, const uint8_t* __restrict__ old, uint8_t* __restrict__ now)
{
    __shared__ int s_e[4][MVHDP_MAXM][2];
    __shared__ double s_u[4][64], s_pa[4][64], s_pb[4][64];
    __shared__ int s_y[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int M = a.M;
    for (int64_t q = (int64_t)blockIdx.x * 4 + wv; q < n_owners; q += (int64_t)gridDim.x * 4) {    // wave-uniform; no barrier in here
        const int64_t d = a.owners[q];
        const uint64_t g = (uint64_t)(a.doc_global0 + d);
        // the entity's side counts of every view, from the old sides
        for (int m = 0; m < M; m++) {
            const int64_t r0 = a.est[(int64_t)m * (a.D + 1) + d], r1 = a.est[(int64_t)m * (a.D + 1) + d + 1];
            int nb = 0;
            for (int64_t c = r0; c < r1; c += 64) {
                const bool in = c + lane < r1;
                const bool b = in && old[a.v[m].rbase + c + lane] != 0;
                nb += __popcll(ballot(b));
            }
            if (lane == 0) { s_e[wv][m][0] = (int)(r1 - r0) - nb; s_e[wv][m][1] = nb; }
        }
        LDS_FENCE();
        for (int m = 0; m < M; m++) {
            const SplitView& v = a.v[m];
            const int64_t r0 = a.est[(int64_t)m * (a.D + 1) + d], r1 = a.est[(int64_t)m * (a.D + 1) + d + 1];
            if (r1 <= r0) continue;
            const int64_t span0 = v.off[d];
            const double Lp_m = (double)(v.off[d + 1] - span0) + v.gas;
            const double pmm = a.P[m * MVHDP_MAXM + m];
            // ---- the pass's constants from the CURRENT side counts of the other views ----
            double sa = 0.0, sb = 0.0;
            for (int i = 0; i < M; i++) {
                if (i == m) continue;
                const int64_t len_i = a.v[i].off[d + 1] - a.v[i].off[d];
                if (len_i == 0) continue;
                const double Lp_i = (double)len_i + a.v[i].gas, p = a.P[m * MVHDP_MAXM + i];
                sa = sa + p * ((double)s_e[wv][i][0] + a.v[i].A) / Lp_i;
                sb = sb + p * ((double)s_e[wv][i][1] + a.v[i].A) / Lp_i;
            }
            const double base_a = v.A + sa * Lp_m, base_b = v.A + sb * Lp_m;
            const int32_t* __restrict__ crow = a.tab + 2 * (a.sumV + m);
            const int ca = crow[0], cb = crow[1];
            const double r0a = 1.0 / ((double)ca + v.beta_sum), r0b = 1.0 / ((double)cb + v.beta_sum);
            const double r1a = 1.0 / ((double)(ca - 1) + v.beta_sum), r1b = 1.0 / ((double)(cb - 1) + v.beta_sum);
            int ea = s_e[wv][m][0], eb = s_e[wv][m][1];
            for (int64_t c = r0; c < r1; c += 64) {
                const int cnt = (int)(r1 - c < 64 ? r1 - c : 64);
                const int64_t idx = v.rbase + c + lane;
                int y = 0;
                if (lane < cnt) {
                    const int64_t pos_n = a.rec_n[idx];
                    const int32_t w = a.rec_w[idx];
                    y = (int)old[idx];
                    const int2 cw = w >= 0 ? *(const int2*)(a.tab + 2 * (v.rowbase + w)) : make_int2(0, 0);
                    s_u[wv][lane] = split_unit(a, g, it, m, (uint32_t)(pos_n - span0));
                    s_pa[wv][lane] = ((double)(cw.x - (y == 0 ? 1 : 0)) + v.beta) * (y == 0 ? r1a : r0a);
                    s_pb[wv][lane] = ((double)(cw.y - (y == 1 ? 1 : 0)) + v.beta) * (y == 1 ? r1b : r0b);
                    s_y[wv][lane] = y;
                }
                LDS_FENCE();
                int mine = y;
                for (int j = 0; j < cnt; j++) {                // the chain: the same on every lane
                    const int yj = s_y[wv][j];
                    if (yj) eb--; else ea--;
                    const double wa = (pmm * (double)ea + base_a) * s_pa[wv][j];
                    const double wb = (pmm * (double)eb + base_b) * s_pb[wv][j];
                    const double total = wa + wb;
                    int s = s_u[wv][j] * total < wa ? 0 : 1;
                    if (total == 0.0 || !(fabs(total) <= 1.7976931348623157e308)) s = yj;
                    if (s) eb++; else ea++;
                    if (j == lane) mine = s;
                }
                LDS_FENCE();
                if (lane < cnt) now[idx] = (uint8_t)mine;
            }
            if (lane == 0) { s_e[wv][m][0] = ea; s_e[wv][m][1] = eb; }
            LDS_FENCE();
        }
    }
}

__global__ __launch_bounds__(256) void split_finish_kernel(const SplitArgs a, const uint8_t* __restrict__ side)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrec || !side[i]) return;
    const int m = view_of(a, i);
    const int64_t n = a.rec_n[i];
    if ((uint64_t)n < (uint64_t)a.v[m].n) a.v[m].z[n] = a.target;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

// every refusal that needs neither the device nor n_k, in the header's order
int split_check(mvhdp_ctx* h, const mvhdp_split_args* a)
{
    const int K = h->mm.K, M = h->mm.M;
    if (!a) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: null args");
    if (a->flags & ~MVHDP_SPLIT_KEEP_ALPHA) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: unknown flags");
    if (a->iterations < 0 || a->iterations > 65535) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: iterations outside 0..65535");
    if (a->source < 0 || a->source >= K) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: source out of range");
    if (a->target < -1 || a->target >= K) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: target out of range");
    if (a->target == a->source) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: source == target");
    const std::string who("split_topic: ");
    if (a->coupling)
        if (const char* r = check_nonneg_finite(a->coupling, (int64_t)M * M)) FAIL(h, MVHDP_ERR_INVALID_ARG, who + "a coupling entry " + r);
    if (a->type_hint)
        for (int m = 0; m < M; m++) {
            if (!a->type_hint[m]) continue;
            for (int w = 0; w < h->mm.V[m]; w++)
                if (a->type_hint[m][w] < -1 || a->type_hint[m][w] > 1) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: a type_hint value outside {-1, 0, 1}");
        }
    if (int rc = require_corpus(h)) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "split_topic before set_hyper");
    if (int rc = require_current_counts(h, "split_topic")) return rc;
    if (h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "split_topic inside an mvhdp_apply_delta_begin bracket (call mvhdp_apply_delta_end first)");
    if (h->mm.mix) FAIL(h, MVHDP_ERR_UNSUPPORTED, "split_topic: a vectors mix is set, and its columns belong to topics (mvhdp_set_vectors_mix(h, 0, NULL, NULL) first)");
    if (mvhdp_emb_has_topic_rows(h)) FAIL(h, MVHDP_ERR_UNSUPPORTED, "split_topic: embeddings with topic rows are initialised (mvhdp_emb_release first)");
    if (K > MVHDP_MAX_TOPICS) FAIL(h, MVHDP_ERR_UNSUPPORTED, "split_topic: more than 2048 topics");
    if (!h->h_inactive.empty() && h->h_inactive[(size_t)a->source]) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: the source is in the inactive set");
    return MVHDP_OK;
}

// the target's conditions (n_k == 0 and alpha == 0.0 in every view); -1: the lowest inactive index that meets them
int split_target(mvhdp_ctx* h, const mvhdp_split_args* a, const std::vector<int32_t>& nk, int32_t& target)
{
    const int K = h->mm.K, M = h->mm.M;
    auto is_free = [&](int t) {
        for (int m = 0; m < M; m++)
            if (nk[(size_t)m * K + t] != 0 || h->h_alpha[(size_t)m * (K + 1) + t] != 0.0) return false;
        return true;
    };
    if (a->target >= 0) {
        if (!is_free(a->target)) FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: the target holds tokens or has alpha != 0 in some view");
        target = a->target;
        return MVHDP_OK;
    }
    for (int t = 0; t < K; t++)
        if (t != a->source && !h->h_inactive.empty() && h->h_inactive[(size_t)t] && is_free(t)) { target = t; return MVHDP_OK; }
    FAIL(h, MVHDP_ERR_INVALID_ARG, "split_topic: no free topic in the inactive set to pick as the target");
}

int split_run(mvhdp_ctx* h, const mvhdp_split_args* a, int64_t* flips_out, mvhdp_split_stats& st)
{
    MvModel& mm = h->mm;
    const int K = mm.K, M = mm.M;
    const int64_t D = mm.D, sumV = mm.rowbase[M], nrows = sumV + M;
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    std::vector<int32_t> nk((size_t)M * K);
    HIPC(h, hipMemcpyAsync(nk.data(), mm.counts + sumV * K, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    int32_t target = -1;
    if (int rc = split_target(h, a, nk, target)) return rc;

    SplitArgs ka{};
    ka.D = D; ka.doc_global0 = mm.doc_id_base; ka.nrows = nrows; ka.sumV = sumV;
    ka.M = M; ka.K = K; ka.source = a->source; ka.target = target;
    ka.seed_lo = (uint32_t)a->seed; ka.seed_hi = (uint32_t)(a->seed >> 32);
    double ah[MVHDP_MAXM];
    for (int m = 0; m < M; m++) {
        SplitView& v = ka.v[m];
        v.off = mm.doc_off[m]; v.tok = mm.tok[m]; v.z = mm.z[m];
        v.n = h->N[m]; v.rowbase = mm.rowbase[m]; v.V = mm.V[m];
        ah[m] = 0.5 * h->h_alpha[(size_t)m * (K + 1) + a->source];
        v.beta = mm.beta[m]; v.beta_sum = mm.beta_sum[m];
        v.A = mm.gamma[m] * ah[m];
        v.gas = mm.gamma[m] * mm.alpha_sum[m];
        for (int i = 0; i < M; i++) {
            double p;
            if (a->coupling) p = a->coupling[m * M + i];
            else if (i == m) p = 1.0;
            else p = mm.p_a[m][i] == 0.0 ? 0.0 : mm.p_a[m][i] / (mm.p_a[m][i] + mm.p_b[m][i]);
            ka.P[m * MVHDP_MAXM + i] = p;
        }
    }
    std::vector<int8_t> hint((size_t)std::max<int64_t>(sumV, 1), (int8_t)-1);
    if (a->type_hint)
        for (int m = 0; m < M; m++)
            if (a->type_hint[m]) memcpy(hint.data() + mm.rowbase[m], a->type_hint[m], (size_t)mm.V[m]);

    // ---- everything that can fail without the handle having changed comes first: the count pass, the lists, the sampler ----
    const int64_t max_blocks = (int64_t)h->num_cus * 8;
    int64_t tpb[MVHDP_MAXM] = {}, nblk[MVHDP_MAXM] = {};
    int64_t blk_total = 0;
    for (int m = 0; m < M; m++) {
        const int64_t ntiles = (h->N[m] + SPLIT_TILE - 1) / SPLIT_TILE;
        if (ntiles == 0) continue;
        tpb[m] = (ntiles + max_blocks - 1) / max_blocks;
        nblk[m] = (ntiles + tpb[m] - 1) / tpb[m];
        blk_total += nblk[m];
    }
    DevArray<int8_t> d_hint;
    DevArray<int64_t> d_blk, d_est, d_rec_n;
    DevArray<int32_t> d_rec_w, d_owners, d_tab;
    DevArray<uint8_t> d_side[2];
    DevArray<unsigned int> d_nown;
    DevArray<u64> d_flips;
    StreamTimer timer;
    HIPC(h, timer.create());
    HIPC(h, d_hint.alloc(hint.size()));
    HIPC(h, d_blk.alloc((size_t)blk_total));
    HIPC(h, d_est.alloc((size_t)M * (size_t)(D + 1)));
    HIPC(h, d_owners.alloc((size_t)D));
    HIPC(h, d_tab.alloc((size_t)nrows * 2));
    HIPC(h, d_nown.alloc(1));
    HIPC(h, d_flips.alloc((size_t)a->iterations + 1));
    HIPC(h, d_hint.upload(hint.data(), hint.size(), s));
    HIPC(h, d_nown.fill(0, s));
    HIPC(h, d_flips.fill(0, s));
    ka.hint = d_hint; ka.est = d_est; ka.owners = d_owners; ka.n_owners = d_nown; ka.tab = d_tab;

    double ms = 0.0, ms_part = 0.0;
    HIPC(h, timer.start(s));
    {
        int64_t b0 = 0;
        for (int m = 0; m < M; m++) {
            if (!nblk[m]) continue;
            LAUNCH(h, split_scan_kernel<false>, dim3((unsigned)nblk[m]), dim3(256), 0, s, ka, m, tpb[m], (const int64_t*)nullptr, d_blk + b0, (uint8_t*)nullptr);
            b0 += nblk[m];
        }
    }
    HIPC(h, timer.stop(s));
    std::vector<int64_t> blk((size_t)blk_total);
    if (blk_total) HIPC(h, d_blk.download(blk.data(), (size_t)blk_total, s));
    HIPC(h, hipStreamSynchronize(s));
    HIPC(h, timer.elapsed_ms(&ms_part));
    ms += ms_part;
    int64_t nrec = 0;
    {
        size_t b = 0;
        for (int m = 0; m < M; m++) {
            ka.v[m].rbase = nrec;
            int64_t in_view = 0;
            for (int64_t j = 0; j < nblk[m]; j++, b++) { const int64_t c = blk[b]; blk[b] = in_view; in_view += c; }   // exclusive, per view
            st.split[m] = in_view;
            nrec += in_view;
        }
    }
    ka.nrec = nrec;
    HIPC(h, d_rec_n.alloc((size_t)nrec));
    HIPC(h, d_rec_w.alloc((size_t)nrec));
    HIPC(h, d_side[0].alloc((size_t)nrec));
    HIPC(h, d_side[1].alloc((size_t)nrec));
    ka.rec_n = d_rec_n; ka.rec_w = d_rec_w;
    if (blk_total) HIPC(h, d_blk.upload(blk.data(), (size_t)blk_total, s));

    HIPC(h, timer.start(s));
    unsigned int n_owners = 0;
    int cur = 0;                                               // the side array that holds the current sides
    LAUNCH(h, split_column_kernel, dim3(blocks_of(nrows)), dim3(256), 0, s, (const int32_t*)mm.counts, nrows, K, a->source, d_tab.get());
    if (nrec > 0) {
        int64_t b0 = 0;
        for (int m = 0; m < M; m++) {
            if (!nblk[m]) continue;
            if (st.split[m]) LAUNCH(h, split_scan_kernel<true>, dim3((unsigned)nblk[m]), dim3(256), 0, s, ka, m, tpb[m], (const int64_t*)(d_blk + b0), (int64_t*)nullptr, d_side[0].get());
            b0 += nblk[m];
        }
        LAUNCH(h, split_csr_kernel, dim3(blocks_of(D + 1)), dim3(256), 0, s, ka);
        LAUNCH(h, split_apply_kernel, dim3(blocks_of(nrec)), dim3(256), 0, s, ka, (const uint8_t*)nullptr, (const uint8_t*)d_side[0].get(), (u64*)nullptr);
        HIPC(h, d_nown.download(&n_owners, 1, s));
        HIPC(h, hipStreamSynchronize(s));
        const unsigned sample_blocks = wave_blocks((int64_t)n_owners, h->num_cus);
        for (int it = 1; it <= a->iterations; it++) {
            LAUNCH(h, split_sample_kernel, dim3(sample_blocks), dim3(256), 0, s, ka, (uint32_t)it, (int64_t)n_owners, (const uint8_t*)d_side[cur].get(), d_side[cur ^ 1].get());
            LAUNCH(h, split_apply_kernel, dim3(blocks_of(nrec)), dim3(256), 0, s, ka, (const uint8_t*)d_side[cur].get(), (const uint8_t*)d_side[cur ^ 1].get(), d_flips + (it - 1));
            cur ^= 1;
        }
    }
    std::vector<u64> flips((size_t)a->iterations + 1, 0);
    std::vector<int32_t> crow((size_t)2 * M, 0);
    HIPC(h, d_flips.download(flips.data(), flips.size(), s));
    HIPC(h, hipMemcpyAsync(crow.data(), d_tab + 2 * sumV, crow.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));                          // the sampler is through: from here on the handle changes

    // ---- the last pass: z, the two columns, alpha and the inactive set ----
    if (nrec > 0) LAUNCH(h, split_finish_kernel, dim3(blocks_of(nrec)), dim3(256), 0, s, ka, (const uint8_t*)d_side[cur].get());
    LAUNCH(h, split_store_kernel, dim3(blocks_of(nrows)), dim3(256), 0, s, mm.counts, nrows, K, a->source, target, (const int32_t*)d_tab.get());
    HIPC(h, timer.stop(s));
    for (int m = 0; m < M; m++)
        if (st.split[m]) h->st.assignments_replaced(m, h->st.view_unassigned(m));
    if (h->st.delta16_used()) {                                // as mvhdp_build_counts: leftovers of a sweep that never reached its apply pass
        HIPC(h, hipMemsetD16Async(mm.delta16, (unsigned short)0x8000, (size_t)(sumV * K), s));
        h->st.delta16_rebiased();
    }
    const std::vector<long long> none((size_t)K, LLONG_MAX);
    HIPC(h, hipMemcpyAsync(h->d_birth_table, none.data(), (size_t)K * sizeof(long long), hipMemcpyHostToDevice, s));
    HIPC(h, hipStreamSynchronize(s));
    HIPC(h, timer.elapsed_ms(&ms_part));
    ms += ms_part;

    for (int m = 0; m < M; m++) {
        if (!(a->flags & MVHDP_SPLIT_KEEP_ALPHA)) h->h_alpha[(size_t)m * (K + 1) + a->source] = ah[m];
        h->h_alpha[(size_t)m * (K + 1) + target] = ah[m];
        st.moved[m] = crow[(size_t)2 * m + 1];
    }
    if (h->h_inactive.empty()) h->h_inactive.assign((size_t)K, 0);
    st.activated = h->h_inactive[(size_t)target] ? 1 : 0;
    h->h_inactive[(size_t)target] = 0;
    mm.first_inactive = -1;
    for (int k = 0; k < K; k++) if (h->h_inactive[(size_t)k]) { mm.first_inactive = k; break; }
    HIPC(h, hipMemcpy(h->d_alpha, h->h_alpha.data(), h->h_alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMemcpy(h->d_inactive, h->h_inactive.data(), (size_t)K, hipMemcpyHostToDevice));
    h->st.counts_rebuilt();                                    // the counts are those of z again; the trees are not those of the counts
    st.target = target;
    st.flips_last = a->iterations > 0 ? (int64_t)flips[(size_t)a->iterations - 1] : 0;
    st.kernel_ms = ms;
    if (flips_out) for (int it = 0; it < a->iterations; it++) flips_out[it] = (int64_t)flips[(size_t)it];
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_split_topic(mvhdp_handle h, const mvhdp_split_args* a, int64_t* flips, mvhdp_split_stats* stats)
{
    CHECK_H(h);
    int rc = split_check(h, a); if (rc) return rc;
    mvhdp_split_stats st{};
    rc = split_run(h, a, flips, st); if (rc) return rc;
    if (stats) *stats = st;
    return MVHDP_OK;
}
