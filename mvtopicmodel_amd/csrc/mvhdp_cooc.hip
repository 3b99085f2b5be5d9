// mvhdp_cooc.hip — mvhdp_word_cooccurrence: in how many windows of a corpus the words of a word set occur, alone and in pairs (include/mvhdp.h
// has the contract).  The integers behind UCI, NPMI and UMass coherence; the formulas themselves stay on the host.  Integers only: no floating
// point anywhere in this file, so integer atomics leave every output exact and the same on every call.
//   cooc_kernel   one wave per entity, longest first, taken from a queue; lanes over positions.  A lane looks its token up in the inverted
//                 index of the sets (first[V + 1], packed (set, slot) memberships) and gets nothing for most tokens of the tail.  An entity
//                 goes in chunks of 64 window starts (a one-window span -- window 0 or a span no longer than the window -- is one chunk of
//                 one start): per touched set a 64-bit mask of the slots present in the chunk and a list of the touched sets, and for a
//                 sliding span per present slot a 64-bit coverage word, bit i = the slot is present in window c + i.  An occurrence at p
//                 covers the starts [p - W + 1, p], so it ORs one run of bits; no window is visited.  Then per touched set one add of
//                 popcount(cov_i & cov_j) per pair of present slots, and the set's words are cleared.
// The per-wave state sits in LDS where it fits, else in a per-wave slice of global memory; either way it is all zero between two chunks.
// co is [n_sets][n][n] of 64-bit cells: a cell never exceeds the number of windows.
#include "mvhdp_side.h"
#include "mvhdp_select.h"

namespace {

enum { CO_BAD = 0, CO_HITS = 1, CO_OOV = 2, CO_QUEUE = 3, CO_WORDS = 4 };
constexpr int64_t COOC_MAX_CELLS = (int64_t)1 << 26;
constexpr int64_t COOC_CHUNK_TOKENS = (int64_t)1 << 24;        // a caller's corpus goes up in chunks of documents of about this many tokens
constexpr int64_t COOC_SLICE_BYTES = (int64_t)1 << 30;         // per-wave global slices of one call, all waves together
constexpr size_t COOC_LDS = 60000;

struct CoocArgs {
    const int64_t* doc_off;                                    // [nd + 1] of the launch's entities
    const int32_t* tok; int64_t tok_shift;                     // token i of the corpus is tok[i - tok_shift]
    const int32_t* order; int64_t nd;                          // the launch's entities, longest first
    int V, n, window; int64_t n_sets;
    const int32_t* first; const uint32_t* memb;                // type w sits in memb[first[w] .. first[w + 1]), each set << 6 | slot
    u64* g_mask; u64* g_cov; int32_t* g_list;                  // per-wave slices [waves][n_sets], [waves][n_sets][n], [waves][n_sets]; null: LDS
    int sliding;                                               // a coverage table exists (some span of the call is longer than the window)
    u64* co; u64* ctl;
};

__device__ __forceinline__ u64 low_bits(int c) { return c >= 64 ? ~0ull : ((1ull << c) - 1ull); }

__global__ __launch_bounds__(256) void cooc_kernel(CoocArgs a)
{
    extern __shared__ u64 cooc_lds[];
    __shared__ int nlists[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, n = a.n;
    const int64_t S = a.n_sets, gw = (int64_t)blockIdx.x * wpb + wave;
    const bool lds = a.g_mask == nullptr;
    u64* mask; u64* cov; int32_t* list;
    if (lds) {
        const int64_t words = S + (a.sliding ? S * n : 0) + (S + 1) / 2;
        mask = cooc_lds + wave * words;
        cov = mask + S;
        list = (int32_t*)(cov + (a.sliding ? S * n : 0));
        for (int64_t i = lane; i < words; i += WAVE) mask[i] = 0;
    } else {
        mask = a.g_mask + gw * S; cov = a.g_cov + gw * S * n; list = a.g_list + gw * S;
    }
    int* nlist = &nlists[wave];
    if (lane == 0) *nlist = 0;
    LDS_FENCE();
    u64 hits = 0, oov = 0;
    bool bad = false;
    for (;;) {
        int64_t q = 0;
        if (lane == 0) q = (int64_t)atomicAdd(&a.ctl[CO_QUEUE], 1ull);
        q = __shfl(q, 0, WAVE);
        if (q >= a.nd) break;
        const int64_t d = a.order[q], b = a.doc_off[d] - a.tok_shift, L = a.doc_off[d + 1] - a.doc_off[d];
        if (L <= 0) continue;
        const int64_t W = a.window;
        const bool one = W == 0 || L <= W;
        const int64_t nwin = one ? 1 : L - W + 1;
        int64_t counted = 0;                                   // the positions below it are in hits and oov already
        for (int64_t c = 0; c < nwin; c += 64) {
            const int nc = (int)min((int64_t)64, nwin - c);
            const int64_t p_hi = one ? L : min(L, c + nc - 1 + W);
            for (int64_t p = c + lane; p < p_hi; p += WAVE) {
                const int t = a.tok[b + p];
                if (t < 0) { bad = true; continue; }
                if (t >= a.V) { if (p >= counted) oov++; continue; }
                const int f0 = a.first[t], f1 = a.first[t + 1];
                if (f1 == f0) continue;
                if (p >= counted) hits++;
                u64 run = 1;                                   // the starts of the chunk whose window holds p
                if (!one) {
                    const int lo = (int)max((int64_t)0, p - W + 1 - c), hi = (int)min((int64_t)nc - 1, p - c);
                    run = low_bits(hi - lo + 1) << lo;
                }
                for (int f = f0; f < f1; f++) {
                    const uint32_t sj = a.memb[f];
                    const int64_t s = sj >> 6;
                    const int j = sj & 63;
                    if (atomicOr(&mask[s], 1ull << j) == 0) list[atomicAdd(nlist, 1)] = (int32_t)s;
                    if (!one) atomicOr(&cov[s * n + j], run);
                }
            }
            counted = p_hi;
            if (lds) LDS_FENCE(); else __threadfence();
            const int nl = *nlist;
            for (int x = lane; x < nl; x += WAVE) {
                const int64_t s = list[x];
                const u64 pm = mask[s];
                u64* cs = cov + s * n;
                u64* cm = a.co + s * n * n;
                for (u64 r = pm; r; r &= r - 1) {
                    const int i = __ffsll((long long)r) - 1;
                    const u64 ci = one ? 1ull : cs[i];
                    atomicAdd(&cm[i * n + i], (u64)__popcll(ci));
                    for (u64 r2 = r & (r - 1); r2; r2 &= r2 - 1) {
                        const int j = __ffsll((long long)r2) - 1;
                        const u64 v = one ? 1ull : (u64)__popcll(ci & cs[j]);
                        if (v) { atomicAdd(&cm[i * n + j], v); atomicAdd(&cm[j * n + i], v); }
                    }
                }
                if (!one) for (u64 r = pm; r; r &= r - 1) cs[__ffsll((long long)r) - 1] = 0;
                mask[s] = 0;
            }
            if (lane == 0) *nlist = 0;
            if (lds) LDS_FENCE(); else __threadfence();
        }
    }
    for (int o = 32; o > 0; o >>= 1) { hits += __shfl_xor(hits, o, WAVE); oov += __shfl_xor(oov, o, WAVE); }
    const bool any_bad = ballot(bad) != 0;
    if (lane == 0) {
        if (hits) atomicAdd(&a.ctl[CO_HITS], hits);
        if (oov) atomicAdd(&a.ctl[CO_OOV], oov);
        if (any_bad) atomicOr(&a.ctl[CO_BAD], 1ull);
    }
}

// the corpus of a call: the caller's host arrays, or the handle's view (off: its host copy of doc_off)
struct Corpus {
    const int64_t* off; const int32_t* tok; int64_t D; bool own;
};

// order = 0 .. n - 1 by span length descending in O(n): a stable counting sort on min(length, 65536), so the spans above that come first in
// index order.  The queue needs no more, and the comparison sort of order_by_length_desc is most of a call's host time at 10^6 entities.
void order_longest_first(std::vector<int32_t>& order, const int64_t* off, int64_t n)
{
    constexpr int64_t CAP = 65536;
    std::vector<int64_t> at((size_t)CAP + 2, 0);
    for (int64_t i = 0; i < n; i++) at[(size_t)(CAP - std::min(off[i + 1] - off[i], CAP)) + 1]++;
    for (int64_t b = 0; b <= CAP; b++) at[(size_t)b + 1] += at[(size_t)b];
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)at[(size_t)(CAP - std::min(off[i + 1] - off[i], CAP))]++] = (int32_t)i;
}

// every check comes before any device work and before the first output is touched; d1 comes back resolved
int check_args(mvhdp_ctx* h, const mvhdp_cooc_args* a, int64_t n_sets, const int32_t* sets, int64_t num_docs, const int64_t* doc_off, const int32_t* tokens,
               const int64_t* co, const int64_t* windows, Corpus& c, int64_t& d1)
{
    MvModel& mm = h->mm;
    if (!a || !co || !windows || n_sets < 0 || (n_sets > 0 && !sets)) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: null args, co, windows or sets, or negative n_sets");
    if (a->m < 0 || a->m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: bad view");
    if (a->n < 1 || a->n > MVHDP_DIAG_MAX_TOP_WORDS) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: n must be 1..64");
    if (a->window < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: negative window");
    const int V = mm.V[a->m];
    if (n_sets > INT64_MAX / a->n) FAIL(h, MVHDP_ERR_UNSUPPORTED, "word_cooccurrence: more than 2^26 cells");
    for (int64_t i = 0; i < n_sets * a->n; i++)
        if (sets[i] < -1 || sets[i] >= V) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: a slot holds neither -1 nor a type of the view");
    if (doc_off) {
        if (num_docs < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: negative num_docs");
        if (const char* r = check_offsets(doc_off, num_docs, INT64_MAX)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("word_cooccurrence: doc_off ") + r);
        if (doc_off[num_docs] > 0 && !tokens) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: null tokens");
        if (const char* r = check_tokens_nonneg(tokens, doc_off[num_docs])) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("word_cooccurrence: ") + r);
        c = Corpus{doc_off, tokens, num_docs, false};
    } else {
        if (!h->have_corpus[a->m]) FAIL(h, MVHDP_ERR_STATE, "word_cooccurrence: no corpus of the view (set_corpus)");
        c = Corpus{h->h_doc_off[a->m].data(), nullptr, (int64_t)h->h_doc_off[a->m].size() - 1, true};
    }
    d1 = a->d1 == -1 ? c.D : a->d1;
    if (a->d0 < 0 || a->d1 < -1 || a->d0 > d1 || d1 > c.D) FAIL(h, MVHDP_ERR_INVALID_ARG, "word_cooccurrence: bad entity range");
    if (n_sets * a->n > COOC_MAX_CELLS / a->n) FAIL(h, MVHDP_ERR_UNSUPPORTED, "word_cooccurrence: more than 2^26 cells");
    return MVHDP_OK;
}

int cooc_run(mvhdp_ctx* h, const mvhdp_cooc_args* a, int64_t S, const int32_t* sets, const Corpus& c, int64_t d1, std::vector<u64>& co, int64_t& windows,
             mvhdp_cooc_stats& st)
{
    MvModel& mm = h->mm;
    const int V = mm.V[a->m], n = a->n;
    const int64_t d0 = a->d0, W = a->window;

    // what the host knows from the spans alone: the windows, the positions, the longest sliding span
    int64_t max_len = 0;
    for (int64_t d = d0; d < d1; d++) {
        const int64_t L = c.off[d + 1] - c.off[d];
        if (L <= 0) continue;
        st.entities++; st.tokens += L;
        windows += (W == 0 || L <= W) ? 1 : L - W + 1;
        max_len = std::max(max_len, L);
    }
    const bool sliding = W > 0 && max_len > W;

    // the inverted index of the sets
    std::vector<int32_t> first((size_t)V + 1, 0);
    for (int64_t i = 0; i < S * n; i++)
        if (sets[i] >= 0) { first[(size_t)sets[i] + 1]++; st.memberships++; }
    for (int w = 0; w < V; w++) { if (first[(size_t)w + 1]) st.distinct_words++; first[(size_t)w + 1] += first[(size_t)w]; }
    std::vector<uint32_t> memb((size_t)st.memberships);
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int64_t s = 0; s < S; s++)
            for (int j = 0; j < n; j++)
                if (sets[s * n + j] >= 0) memb[(size_t)at[(size_t)sets[s * n + j]]++] = (uint32_t)(s << 6) | (uint32_t)j;
    }

    if (int rc = side_begin(h)) return rc;
    hipStream_t s = h->stream;
    if (d1 == d0) return MVHDP_OK;

    // the per-wave state: LDS where a block of 4, 2 or 1 waves fits, else slices of global memory for as many waves as the budget holds
    const int64_t wave_words = S + (sliding ? S * n : 0) + (S + 1) / 2;
    int wpb = 4;
    while (wpb > 1 && (size_t)(wpb * wave_words) * 8 > COOC_LDS) wpb >>= 1;
    const bool lds = (size_t)(wpb * wave_words) * 8 <= COOC_LDS;
    int64_t max_waves = (int64_t)h->num_cus * 16 * 4;
    if (!lds) { max_waves = std::max<int64_t>(1, std::min(max_waves, COOC_SLICE_BYTES / (wave_words * 8))); wpb = (int)std::min<int64_t>(4, max_waves); }

    DevArray<int32_t> d_first, d_list, d_order, d_tok;
    DevArray<uint32_t> d_memb;
    DevArray<u64> d_mask, d_cov, d_co, d_ctl;
    DevArray<int64_t> d_off;
    HIPC(h, d_first.alloc(first.size()));
    HIPC(h, d_memb.alloc(memb.size()));
    HIPC(h, d_co.alloc((size_t)(S * n * n)));
    HIPC(h, d_ctl.alloc(CO_WORDS));
    HIPC(h, d_first.upload(first.data(), first.size(), s));
    if (!memb.empty()) HIPC(h, d_memb.upload(memb.data(), memb.size(), s));
    HIPC(h, d_co.fill(0, s));
    HIPC(h, d_ctl.fill(0, s));
    if (!lds) {
        const int64_t slices = (max_waves / wpb) * wpb;
        HIPC(h, d_mask.alloc((size_t)(slices * S)));
        HIPC(h, d_list.alloc((size_t)(slices * S)));
        HIPC(h, d_cov.alloc(sliding ? (size_t)(slices * S * n) : 0));
        HIPC(h, d_mask.fill(0, s));
        if (sliding) HIPC(h, d_cov.fill(0, s));
    }
    const size_t lds_bytes = lds ? (size_t)(wpb * wave_words) * 8 : 0;
    HIPC(h, hipFuncSetAttribute((const void*)cooc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(lds_bytes, 1)));
    StreamTimer timer;
    HIPC(h, timer.create());

    CoocArgs ca{};
    ca.V = V; ca.n = n; ca.window = a->window; ca.n_sets = S;
    ca.first = d_first; ca.memb = d_memb;
    ca.g_mask = lds ? nullptr : d_mask.get(); ca.g_cov = lds ? nullptr : d_cov.get(); ca.g_list = lds ? nullptr : d_list.get();
    ca.sliding = sliding ? 1 : 0;
    ca.co = d_co; ca.ctl = d_ctl;

    // the handle's corpus is one launch; a caller's goes up in chunks of whole documents (MVHDP_COOC_CHUNK_TOKENS: the tests' chunk size)
    int64_t chunk_tokens = COOC_CHUNK_TOKENS;
    if (const char* e = getenv("MVHDP_COOC_CHUNK_TOKENS")) { const long long v = atoll(e); if (v > 0) chunk_tokens = v; }
    std::vector<int32_t> order;
    for (int64_t c0 = d0; c0 < d1;) {
        int64_t c1 = d1;
        if (!c.own) {
            c1 = c0 + 1;
            while (c1 < d1 && c1 - c0 < INT32_MAX && c.off[c1 + 1] - c.off[c0] <= chunk_tokens) c1++;
        } else if (c1 - c0 > INT32_MAX) c1 = c0 + INT32_MAX;
        const int64_t nd = c1 - c0, nt = c.off[c1] - c.off[c0];
        order_longest_first(order, c.off + c0, nd);
        HIPC(h, d_order.alloc((size_t)nd));
        HIPC(h, d_order.upload(order.data(), (size_t)nd, s));
        if (c.own) {
            ca.doc_off = mm.doc_off[a->m] + c0; ca.tok = mm.tok[a->m]; ca.tok_shift = 0;
        } else {
            HIPC(h, d_off.alloc((size_t)nd + 1));
            HIPC(h, d_tok.alloc((size_t)nt));
            HIPC(h, d_off.upload(c.off + c0, (size_t)nd + 1, s));
            if (nt > 0) HIPC(h, d_tok.upload(c.tok + c.off[c0], (size_t)nt, s));
            ca.doc_off = d_off; ca.tok = d_tok; ca.tok_shift = c.off[c0];
        }
        ca.order = d_order; ca.nd = nd;
        HIPC(h, hipMemsetAsync(d_ctl.get() + CO_QUEUE, 0, sizeof(u64), s));
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min((nd + wpb - 1) / wpb, max_waves / wpb));
        HIPC(h, timer.start(s));
        LAUNCH(h, cooc_kernel, dim3(grid), dim3(64 * wpb), lds_bytes, s, ca);
        HIPC(h, timer.stop(s));
        HIPC(h, hipStreamSynchronize(s));                      // the chunk's staging arrays are free again
        double ms = 0.0;
        HIPC(h, timer.elapsed_ms(&ms));
        st.kernel_ms += ms;
        c0 = c1;
    }
    u64 ctl[CO_WORDS] = {};
    HIPC(h, d_ctl.download(ctl, CO_WORDS, s));
    co.resize((size_t)(S * n * n));
    if (!co.empty()) HIPC(h, d_co.download(co.data(), co.size(), s));
    HIPC(h, hipStreamSynchronize(s));
    if (ctl[CO_BAD]) FAIL(h, MVHDP_ERR_STATE, "word_cooccurrence: a token of the range has a negative type");
    st.hits = (int64_t)ctl[CO_HITS];
    st.oov = (int64_t)ctl[CO_OOV];
    return MVHDP_OK;
}

} // namespace

extern "C" int mvhdp_word_cooccurrence(mvhdp_handle h, const mvhdp_cooc_args* a, int64_t n_sets, const int32_t* sets, int64_t num_docs, const int64_t* doc_off,
                                       const int32_t* tokens, int64_t* co, int64_t* windows, mvhdp_cooc_stats* stats)
{
    CHECK_H(h);
    Corpus c{};
    int64_t d1 = 0;
    int rc = check_args(h, a, n_sets, sets, num_docs, doc_off, tokens, co, windows, c, d1); if (rc) return rc;
    mvhdp_cooc_stats st{};
    std::vector<u64> out;
    int64_t nwin = 0;
    rc = cooc_run(h, a, n_sets, sets, c, d1, out, nwin, st); if (rc) return rc;
    // everything is known: now the caller's arrays (an empty range leaves co all zero)
    const size_t cells = (size_t)(n_sets * a->n * a->n);
    if (out.empty()) memset(co, 0, cells * sizeof(int64_t)); else memcpy(co, out.data(), cells * sizeof(int64_t));
    *windows = nwin;
    if (stats) *stats = st;
    return MVHDP_OK;
}
