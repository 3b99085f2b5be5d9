// mvhdp_cohort.hip — mvhdp_cohort_top_words: a topic's words inside a set of entities (include/mvhdp.h has the contract).  A cohort is a
// list of entity ids; per cohort g and topic k the call counts the view-m tokens of type w and topic k over the cohort's listings,
// c_g[w][k], and returns the top n types by count or by the share c_g[w][k] / n_wk[w][k], with tokens[g][k], docs[g][k], nonzero[g][k].
// Integers only: no floating point anywhere in this file, so integer atomics leave every output exact and the same on every call.
//   cohort_count_kernel<TABLE>   one wave per listing, lanes over the span's tokens: validates type and z, counts the listing's tokens per
//                                topic in the wave's LDS row, and with TABLE adds every counted token into the cohort's [K][V_m] table
//                                (topic-major, so that the selection reads a topic's column contiguously); at the listing's end one
//                                atomic per topic seen into tokens[g][k] and one into docs[g][k].  Without TABLE: the trends-only call.
//   cohort_select_kernel<Ord>    one block per (cohort of the pass, topic), the shape of diag_topn_kernel: a sorted top-n list per wave in
//                                registers (topn_offer, mvhdp_select.h), the four lists merged by wave 0.  CountOrder: the keys of
//                                mvhdp_top_words.  ShareOrder: an entry carries the handle's n_wk cell beside its key, read only for the
//                                types that reach min_count, and two entries compare by 64-bit cross products.
// The cohorts go in passes of as many tables as fit scratch_bytes; a pass clears its tables, counts its listings and selects.
#include "mvhdp_side.h"
#include "mvhdp_select.h"

namespace {

enum { CH_BAD = 0, CH_SKIPPED = 1, CH_TOKENS = 2, CH_WORDS = 3 };
constexpr int64_t COHORT_SCRATCH_DEFAULT = (int64_t)1 << 30;   // count tables of a pass when scratch_bytes == 0
constexpr size_t COHORT_LDS = 65536;

struct CohortCountArgs {
    const int64_t* doc_off; const int32_t* tok; const int32_t* z;
    const int64_t* member_off; const int64_t* members;         // of the whole call
    int64_t g0; int nb;                                        // the pass: cohorts [g0, g0 + nb)
    int64_t q0, q1;                                            //   and their listings [member_off[g0], member_off[g0 + nb])
    int K, V;
    int32_t* table;                                            // [nb][K][V], zero (TABLE only)
    u64* tokens; u64* docs;                                    // [G][K]
    u64* ctl;                                                  // CH_*
};

template <bool TABLE>
__global__ __launch_bounds__(256) void cohort_count_kernel(CohortCountArgs a)
{
    extern __shared__ int32_t cohort_lds[];                    // [waves of the block][K]: the listing's tokens per topic
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, K = a.K;
    int32_t* cnt = cohort_lds + (size_t)wave * K;
    for (int k = lane; k < K; k += WAVE) cnt[k] = 0;
    LDS_FENCE();
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    u64 skipped = 0, counted = 0;
    bool bad = false;
    for (int64_t q = a.q0 + (int64_t)blockIdx.x * wpb + wave; q < a.q1; q += nwaves) {
        int lo = 0, hi = a.nb;                                 // the listing's cohort: member_off[g0 + lo] <= q < member_off[g0 + hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.member_off[a.g0 + mid] <= q) lo = mid; else hi = mid;
        }
        const int64_t d = a.members[q], b = a.doc_off[d], e = a.doc_off[d + 1];
        int32_t* tab = a.table + (int64_t)lo * K * a.V;
        for (int64_t i = b + lane; i < e; i += WAVE) {
            const int t = a.tok[i], zz = a.z[i];
            if (zz < -1 || zz >= K || t < 0) { bad = true; continue; }
            if (zz < 0 || t >= a.V) { skipped++; continue; }
            atomicAdd(&cnt[zz], 1);
            if (TABLE) atomicAdd(&tab[(int64_t)zz * a.V + t], 1);
        }
        LDS_FENCE();
        u64* tk = a.tokens + (a.g0 + lo) * K;
        u64* dc = a.docs + (a.g0 + lo) * K;
        for (int k = lane; k < K; k += WAVE) {
            const int c = cnt[k];
            if (c == 0) continue;
            atomicAdd(&tk[k], (u64)c);
            atomicAdd(&dc[k], 1ull);
            counted += (u64)c;
            cnt[k] = 0;
        }
        LDS_FENCE();
    }
    for (int o = 32; o > 0; o >>= 1) { skipped += __shfl_xor(skipped, o, WAVE); counted += __shfl_xor(counted, o, WAVE); }
    const bool any_bad = ballot(bad) != 0;
    if (lane == 0) {
        if (skipped) atomicAdd(&a.ctl[CH_SKIPPED], skipped);
        if (counted) atomicAdd(&a.ctl[CH_TOKENS], counted);
        if (any_bad) atomicOr(&a.ctl[CH_BAD], 1ull);
    }
}

// MVHDP_COHORT_BY_COUNT: the key (count << 32 | type) of diag_topn_kernel, larger first
__device__ __forceinline__ u64 count_key(int c, int w) { return ((u64)(uint32_t)c << 32) | (uint32_t)w; }
struct CountOrder : KeyDescending {
    typedef u64 entry;
    static __device__ __forceinline__ u64 empty() { return 0; }
    static __device__ __forceinline__ u64 make(int c, int w, const int32_t*) { return count_key(c, w); }
    static __device__ __forceinline__ u64 key(u64 e) { return e; }
};

// MVHDP_COHORT_BY_SHARE: c / all descending by cross products (c, all < 2^31: a product is below 2^62), equal shares by the key.  The
// empty entry (0, 0) ties every share and loses on the key, so it stays behind every real entry.
struct ShareEntry { u64 key; uint32_t all; };                  // all: n_wk of the type and topic
__device__ __forceinline__ ShareEntry lane_get(const ShareEntry& v, int j) { return ShareEntry{__shfl(v.key, j, WAVE), __shfl(v.all, j, WAVE)}; }
__device__ __forceinline__ ShareEntry lane_up1(const ShareEntry& v) { return ShareEntry{__shfl_up(v.key, 1, WAVE), __shfl_up(v.all, 1, WAVE)}; }
struct ShareOrder {
    typedef ShareEntry entry;
    __device__ __forceinline__ bool operator()(const ShareEntry& a, const ShareEntry& b) const
    {
        const u64 l = (a.key >> 32) * (u64)b.all, r = (b.key >> 32) * (u64)a.all;
        return l > r || (l == r && a.key > b.key);
    }
    static __device__ __forceinline__ ShareEntry empty() { return ShareEntry{0, 0}; }
    static __device__ __forceinline__ ShareEntry make(int c, int w, const int32_t* nwk_cell) { return ShareEntry{count_key(c, w), (uint32_t)*nwk_cell}; }
    static __device__ __forceinline__ u64 key(const ShareEntry& e) { return e.key; }
};

// table: the pass's [nb][K][V]; nwk: the handle's n_wk of the view, [V][K]; the outputs start at the pass's first cohort
template <class Ord>
__global__ __launch_bounds__(256) void cohort_select_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ nwk, int V, int K, int n, int min_count,
                                                            int32_t* __restrict__ types, int32_t* __restrict__ counts, int32_t* __restrict__ nonzero)
{
    typedef typename Ord::entry Entry;
    __shared__ Entry lists[4][64];
    __shared__ int nzs[4];
    const int64_t cell = blockIdx.x;                           // (cohort of the pass, topic)
    const int k = (int)(cell % K), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* col = table + cell * V;
    const int per = (V + 3) / 4, b = wave * per, e = min(V, b + per);
    Entry list = Ord::empty(), thr = Ord::empty();
    int nz = 0;
    for (int base = b; base < e; base += WAVE) {
        const int w = base + lane;
        Entry key = Ord::empty();
        if (w < e) {
            const int c = col[w];
            if (c > 0) nz++;
            if (c >= min_count) key = Ord::make(c, w, nwk + (int64_t)w * K + k);
        }
        if (ballot(Ord()(key, thr))) topn_offer(list, thr, key, n, lane, Ord());
    }
    for (int o = 32; o >= 1; o >>= 1) nz += __shfl_xor(nz, o, WAVE);
    lists[wave][lane] = list;
    if (lane == 0) nzs[wave] = nz;
    __syncthreads();
    if (wave != 0) return;
    for (int w2 = 1; w2 < 4; w2++) topn_offer(list, thr, lists[w2][lane], n, lane, Ord());
    if (lane < n) {
        const u64 key = Ord::key(list);
        types[cell * n + lane] = key ? (int32_t)(uint32_t)key : -1;          // unfilled slots: -1 / 0
        counts[cell * n + lane] = (int32_t)(key >> 32);
    }
    if (lane == 0) nonzero[cell] = nzs[0] + nzs[1] + nzs[2] + nzs[3];
}

// every check comes before any device work and before the first output is touched
int check_args(mvhdp_ctx* h, const mvhdp_cohort_args* a, int64_t G, const int64_t* member_off, const int64_t* members, const int32_t* types, const int32_t* counts)
{
    MvModel& mm = h->mm;
    if (!a || G < 0 || !member_off) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: null args or member_off, or negative n_cohorts");
    if (a->m < 0 || a->m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: bad view");
    if (a->n < 1 || a->n > MVHDP_DIAG_MAX_TOP_WORDS) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: n must be 1..64");
    if (a->order != MVHDP_COHORT_BY_COUNT && a->order != MVHDP_COHORT_BY_SHARE) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: bad order");
    if (a->min_count < 1 || a->scratch_bytes < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: min_count < 1 or negative scratch_bytes");
    if ((types == nullptr) != (counts == nullptr)) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: types and counts go together");
    if (const char* r = check_offsets(member_off, G, INT64_MAX)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("cohort_top_words: member_off ") + r);
    if (member_off[G] > 0 && !members) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: null members");
    if (!h->have_corpus[a->m]) FAIL(h, MVHDP_ERR_STATE, "cohort_top_words: no corpus of the view (set_corpus)");
    if (a->order == MVHDP_COHORT_BY_SHARE)
        if (int rc = require_current_counts(h, "cohort_top_words: BY_SHARE needs current counts")) return rc;
    const std::vector<int64_t>& off = h->h_doc_off[a->m];
    for (int64_t g = 0; g < G; g++) {
        int64_t span = 0;
        for (int64_t q = member_off[g]; q < member_off[g + 1]; q++) {
            const int64_t d = members[q];
            if (d < 0 || d >= mm.D) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: member outside [0, D)");
            span += off[(size_t)d + 1] - off[(size_t)d];
            if (span > INT32_MAX) FAIL(h, MVHDP_ERR_INVALID_ARG, "cohort_top_words: the listings of one cohort hold more than 2^31 - 1 tokens");
        }
    }
    if (mm.K > (int)(COHORT_LDS / sizeof(int32_t))) FAIL(h, MVHDP_ERR_UNSUPPORTED, "cohort_top_words: more than 16384 topics");
    return MVHDP_OK;
}

struct CohortOut {
    std::vector<int32_t> types, counts, nonzero;
    std::vector<u64> tokens, docs;
};

int cohort_run(mvhdp_ctx* h, const mvhdp_cohort_args* a, int64_t G, const int64_t* member_off, const int64_t* members, bool want_lists, bool want_nz,
               CohortOut& out, mvhdp_cohort_stats& st)
{
    MvModel& mm = h->mm;
    const int K = mm.K, V = mm.V[a->m], n = a->n;
    const int64_t nm = member_off[G], cells = (int64_t)K * V;
    const bool table = want_lists || want_nz;
    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;

    // cohorts per pass: the tables that fit the scratch, at least one; a pass's (cohort, topic) cells within one grid
    int64_t B = G;
    if (table && cells > 0) B = std::max<int64_t>(1, (a->scratch_bytes > 0 ? a->scratch_bytes : COHORT_SCRATCH_DEFAULT) / (cells * (int64_t)sizeof(int32_t)));
    B = std::max<int64_t>(1, std::min(std::min(B, G), (int64_t)INT32_MAX / K));

    DevArray<int64_t> d_moff, d_mem;
    DevArray<u64> d_tokens, d_docs, d_ctl;
    DevArray<int32_t> d_table, d_types, d_counts, d_nz;
    HIPC(h, d_moff.alloc((size_t)G + 1));
    HIPC(h, d_mem.alloc((size_t)nm));
    HIPC(h, d_tokens.alloc((size_t)(G * K)));
    HIPC(h, d_docs.alloc((size_t)(G * K)));
    HIPC(h, d_ctl.alloc(CH_WORDS));
    HIPC(h, d_moff.upload(member_off, (size_t)G + 1, s));
    if (nm > 0) HIPC(h, d_mem.upload(members, (size_t)nm, s));
    HIPC(h, d_tokens.fill(0, s));
    HIPC(h, d_docs.fill(0, s));
    HIPC(h, d_ctl.fill(0, s));
    if (table) {
        HIPC(h, d_table.alloc((size_t)(B * cells)));
        HIPC(h, d_types.alloc((size_t)(G * K * n)));
        HIPC(h, d_counts.alloc((size_t)(G * K * n)));
        HIPC(h, d_nz.alloc((size_t)(G * K)));
    }
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * K * sizeof(int32_t) > COHORT_LDS) wpb >>= 1;
    const size_t lds = (size_t)wpb * K * sizeof(int32_t);
    HIPC(h, hipFuncSetAttribute((const void*)cohort_count_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPC(h, hipFuncSetAttribute((const void*)cohort_count_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    StreamTimer timer;
    HIPC(h, timer.create());
    HIPC(h, timer.start(s));

    const int32_t* nwk = mm.counts + mm.rowbase[a->m] * K;
    for (int64_t g0 = 0; g0 < G; g0 += B) {
        const int64_t nb = std::min(B, G - g0), q0 = member_off[g0], q1 = member_off[g0 + nb];
        if (table && cells > 0) HIPC(h, hipMemsetAsync(d_table.get(), 0, (size_t)(nb * cells) * sizeof(int32_t), s));
        if (q1 > q0) {
            CohortCountArgs ca{};
            ca.doc_off = mm.doc_off[a->m]; ca.tok = mm.tok[a->m]; ca.z = mm.z[a->m];
            ca.member_off = d_moff; ca.members = d_mem;
            ca.g0 = g0; ca.nb = (int)nb; ca.q0 = q0; ca.q1 = q1;
            ca.K = K; ca.V = V;
            ca.table = d_table; ca.tokens = d_tokens; ca.docs = d_docs; ca.ctl = d_ctl;
            const unsigned grid = (unsigned)std::min<int64_t>((q1 - q0 + wpb - 1) / wpb, (int64_t)h->num_cus * 8);
            if (table) LAUNCH(h, cohort_count_kernel<true>, dim3(grid), dim3(64 * wpb), lds, s, ca);
            else LAUNCH(h, cohort_count_kernel<false>, dim3(grid), dim3(64 * wpb), lds, s, ca);
        }
        if (table) {
            int32_t* ty = d_types + g0 * K * n;
            int32_t* co = d_counts + g0 * K * n;
            int32_t* nz = d_nz + g0 * K;
            if (a->order == MVHDP_COHORT_BY_SHARE)
                LAUNCH(h, cohort_select_kernel<ShareOrder>, dim3((unsigned)(nb * K)), dim3(256), 0, s, d_table.get(), nwk, V, K, n, a->min_count, ty, co, nz);
            else
                LAUNCH(h, cohort_select_kernel<CountOrder>, dim3((unsigned)(nb * K)), dim3(256), 0, s, d_table.get(), nwk, V, K, n, a->min_count, ty, co, nz);
        }
        st.passes++;
    }
    HIPC(h, timer.stop(s));
    u64 ctl[CH_WORDS] = {};
    HIPC(h, d_ctl.download(ctl, CH_WORDS, s));
    HIPC(h, hipStreamSynchronize(s));
    if (ctl[CH_BAD]) FAIL(h, MVHDP_ERR_STATE, "cohort_top_words: a listed token has a topic outside [-1, K) or a negative type");
    out.tokens.resize((size_t)(G * K)); out.docs.resize((size_t)(G * K));
    HIPC(h, d_tokens.download(out.tokens.data(), out.tokens.size(), s));
    HIPC(h, d_docs.download(out.docs.data(), out.docs.size(), s));
    if (want_lists) {
        out.types.resize((size_t)(G * K * n)); out.counts.resize((size_t)(G * K * n));
        HIPC(h, d_types.download(out.types.data(), out.types.size(), s));
        HIPC(h, d_counts.download(out.counts.data(), out.counts.size(), s));
    }
    if (want_nz) {
        out.nonzero.resize((size_t)(G * K));
        HIPC(h, d_nz.download(out.nonzero.data(), out.nonzero.size(), s));
    }
    HIPC(h, hipStreamSynchronize(s));
    HIPC(h, timer.elapsed_ms(&st.kernel_ms));
    st.listings = nm;
    st.tokens = (int64_t)ctl[CH_TOKENS];
    st.skipped = (int64_t)ctl[CH_SKIPPED];
    st.cohorts_per_pass = (int32_t)std::min<int64_t>(B, INT32_MAX);
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_cohort_top_words(mvhdp_handle h, const mvhdp_cohort_args* a, int64_t n_cohorts, const int64_t* member_off, const int64_t* members,
                                      int32_t* types, int32_t* counts, int32_t* nonzero, int64_t* tokens, int64_t* docs, mvhdp_cohort_stats* stats)
{
    CHECK_H(h);
    int rc = check_args(h, a, n_cohorts, member_off, members, types, counts); if (rc) return rc;
    mvhdp_cohort_stats st{};
    if (n_cohorts == 0) { if (stats) *stats = st; return MVHDP_OK; }
    CohortOut out;
    rc = cohort_run(h, a, n_cohorts, member_off, members, types != nullptr, nonzero != nullptr, out, st); if (rc) return rc;
    // everything is known: now the caller's arrays
    if (types) memcpy(types, out.types.data(), out.types.size() * sizeof(int32_t));
    if (counts) memcpy(counts, out.counts.data(), out.counts.size() * sizeof(int32_t));
    if (nonzero) memcpy(nonzero, out.nonzero.data(), out.nonzero.size() * sizeof(int32_t));
    if (tokens) memcpy(tokens, out.tokens.data(), out.tokens.size() * sizeof(int64_t));
    if (docs) memcpy(docs, out.docs.data(), out.docs.size() * sizeof(int64_t));
    if (stats) *stats = st;
    return MVHDP_OK;
}
