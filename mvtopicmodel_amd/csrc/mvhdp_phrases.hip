// mvhdp_phrases.hip — findTopicPhrases (PTM:1921-1976) on the device: the same-topic word runs of the view-0 tokens, counted per topic
// (include/mvhdp.h has the contract).  Integers only: no floating point anywhere in this file.
//   phrase_walk_kernel<false>   one wave per entity, 64 positions a step: validates tokens and z, counts runs, and the phrase occurrences
//                               of every wave of the grid
//   phrase_walk_kernel<true>    the same walk by the same grid; writes one record per occurrence (topic, start, length, hash), every wave
//                               into the room its own count asked for -- no atomic (one per step on a single counter cost 27 ms at C4)
//   phrase_insert_kernel        one thread per record into an open-addressing table of twice as many slots (it cannot fill): the hash places,
//                               the corpus decides -- two records are one phrase iff topic, length and every word id are equal
//   phrase_scatter_kernel       the used slots grouped by topic (the segment bounds are the prefix sums of distinct[k])
//   phrase_select_kernel        one block per topic: the count of its max_per_topic-th most frequent phrase (a bitwise descent over the
//                               segment), how many phrases reach it, and the sum of all its counts (countssum, PTM:2037)
//   phrase_pack_kernel          those phrases -- the kept ones and the count ties at the cut -- next to each other
//   phrase_words_kernel         their word ids, gathered from the corpus
// The host settles the order inside equal counts (word ids, ascending lexicographic, a proper prefix first) and cuts.  Which occurrence
// represents a phrase, and where it sits in the table, depends on the schedule; the output does not: every occurrence of a phrase has the
// same words, and the final order is total.
//
// The walk.  The reference's loop is a three-state automaton over the positions of one entity: EMPTY (prevtopic = -1), HOLD (prevtopic =
// the topic of the token before, no phrase open), OPEN (a phrase is open).  A token whose topic equals the token before it sends
// EMPTY -> HOLD, HOLD -> OPEN, OPEN -> OPEN; any other token sends EMPTY -> HOLD, HOLD -> HOLD, OPEN -> EMPTY and, from OPEN, counts the
// phrase (the token itself is swallowed).  A map of three states to three states takes six bits and maps compose associatively, so a wave
// resolves 64 positions with one inclusive scan and carries one state to the next 64.  A phrase starts at the last position that left
// the automaton in HOLD and ends in front of the token that broke it; nothing is flushed at the end of the entity.
#include "mvhdp_ctx.h"
#include "mvhdp_select.h"

namespace {

constexpr int WV = 64;

enum : int { ST_EMPTY = 0, ST_HOLD = 1, ST_OPEN = 2 };
// state s maps to (map >> 2 s) & 3
constexpr int MAP_SAME = ST_HOLD | (ST_OPEN << 2) | (ST_OPEN << 4);
constexpr int MAP_OTHER = ST_HOLD | (ST_HOLD << 2) | (ST_EMPTY << 4);
constexpr int MAP_ID = ST_EMPTY | (ST_HOLD << 2) | (ST_OPEN << 4);

enum { PH_RUNS = 0, PH_BAD = 1, PH_COLLISIONS = 2, PH_WORDS = 3 };
constexpr u64 SLOT_FREE = ~0ull;

struct PhraseRec { int64_t start; u64 hash; int32_t topic, len; };   // start: index into the view-0 tokens

__device__ __forceinline__ int compose(int later, int earlier)  // later after earlier
{
    return ((later >> (2 * (earlier & 3))) & 3) | (((later >> (2 * ((earlier >> 2) & 3))) & 3) << 2) | (((later >> (2 * ((earlier >> 4) & 3))) & 3) << 4);
}

__device__ __forceinline__ u64 mix64(u64 x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

__device__ u64 phrase_hash(const int32_t* __restrict__ tok, int64_t start, int32_t len, int32_t topic)
{
    u64 h = mix64(((u64)(uint32_t)topic << 32) | (u64)(uint32_t)len);
    for (int32_t i = 0; i < len; i++) h = (h ^ (u64)(uint32_t)tok[start + i]) * 0x9e3779b97f4a7c15ull + (h >> 29);
    return mix64(h);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void phrase_walk_kernel(const int64_t* __restrict__ doc_off, const int32_t* __restrict__ tok, const int32_t* __restrict__ z,
                                                          int64_t D, int K, int V0, u64* __restrict__ ctl, u64* __restrict__ wave_room /*[waves of the grid]*/,
                                                          PhraseRec* __restrict__ rec, u64 rec_cap)
{
    const int lane = threadIdx.x & (WV - 1);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / WV) + (threadIdx.x / WV), nwaves = (int64_t)gridDim.x * (blockDim.x / WV);
    const u64 below = (1ull << lane) - 1ull;
    u64 runs = 0, occ = 0;                                     // occ: the count pass counts; the write pass starts at the sum of the waves before this one
    if (WRITE) occ = wave_room[wave];
    bool bad = false;
    for (int64_t d = wave; d < D; d += nwaves) {               // wave-uniform from here on, but for the hash loop
        const int64_t b = doc_off[d], e = doc_off[d + 1];
        int st = ST_EMPTY, carry_topic = -1;
        int64_t carry_start = -1;
        for (int64_t base = b; base < e; base += WV) {
            const int64_t pos = base + lane;
            const bool in = pos < e;
            const int32_t t = in ? z[pos] : -2;
            const int32_t w = in ? tok[pos] : 0;
            bad = bad || (in && ((uint32_t)t >= (uint32_t)K || (uint32_t)w >= (uint32_t)V0));
            int32_t tp = __shfl_up(t, 1);
            if (lane == 0) tp = carry_topic;
            const bool same = in && t == tp;
            int map = !in ? MAP_ID : same ? MAP_SAME : MAP_OTHER;
#pragma unroll
            for (int o = 1; o < WV; o <<= 1) {
                const int other = __shfl_up(map, o);
                if (lane >= o) map = compose(map, other);
            }
            const int post = (map >> (2 * st)) & 3;            // the state this position leaves behind
            int pre = __shfl_up(post, 1);
            if (lane == 0) pre = st;
            const bool emit = in && !same && pre == ST_OPEN;
            runs += (u64)__popcll(ballot(in && !same));
            const u64 hold = ballot(in && post == ST_HOLD);
            const u64 em = ballot(emit);
            if (WRITE && em) {
                const u64 at = occ + (u64)__popcll(em & below);
                const u64 hb = hold & below;
                const int64_t start = hb ? base + (63 - __clzll((long long)hb)) : carry_start;
                if (emit && at < rec_cap && start >= b) {
                    const int32_t len = (int32_t)(pos - start);
                    PhraseRec r;
                    r.start = start; r.len = len; r.topic = tp; r.hash = phrase_hash(tok, start, len, tp);
                    rec[at] = r;
                }
            }
            occ += (u64)__popcll(em);
            st = __shfl(post, WV - 1);
            carry_topic = __shfl(t, WV - 1);
            if (hold) carry_start = base + (63 - __clzll((long long)hold));
        }
    }
    if (!WRITE) {
        const bool any_bad = ballot(bad) != 0;
        if (lane == 0) {
            if (runs) atomicAdd(&ctl[PH_RUNS], runs);
            wave_room[wave] = occ;
            if (any_bad) atomicOr(&ctl[PH_BAD], 1ull);
        }
    }
}

__device__ bool same_phrase(const int32_t* __restrict__ tok, const PhraseRec& a, const PhraseRec& b)
{
    if (a.topic != b.topic || a.len != b.len) return false;
    if (a.start == b.start) return true;
    for (int32_t i = 0; i < a.len; i++)
        if (tok[a.start + i] != tok[b.start + i]) return false;
    return true;
}

// slot_rec[p]: the record that claimed slot p (SLOT_FREE: none); slot_cnt[p]: the occurrences of its phrase.  cap_mask + 1 >= 2 n slots.
__global__ __launch_bounds__(256) void phrase_insert_kernel(const PhraseRec* __restrict__ rec, u64 n, const int32_t* __restrict__ tok, u64 hash_mask,
                                                            u64* slot_rec, uint32_t* slot_cnt, u64 cap_mask, u64* distinct /*[K]*/, u64* ctl)
{
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 coll = 0;
    if (r < n) {
        const PhraseRec me = rec[r];
        const u64 uh = me.hash & hash_mask;
        u64 p = (uh ^ (uh >> 32)) & cap_mask;
        for (;;) {
            u64 cur = __hip_atomic_load(&slot_rec[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == SLOT_FREE) {
                cur = atomicCAS(&slot_rec[p], SLOT_FREE, r);
                if (cur == SLOT_FREE) { atomicAdd(&slot_cnt[p], 1u); atomicAdd(&distinct[me.topic], 1ull); break; }
            }
            const PhraseRec other = rec[cur];                  // the records were complete before this kernel started
            if ((other.hash & hash_mask) == uh) {
                if (same_phrase(tok, me, other)) { atomicAdd(&slot_cnt[p], 1u); break; }
                coll++;
            }
            p = (p + 1) & cap_mask;
        }
    }
    for (int o = 32; o > 0; o >>= 1) coll += __shfl_xor(coll, o);
    if ((threadIdx.x & (WV - 1)) == 0 && coll) atomicAdd(&ctl[PH_COLLISIONS], coll);
}

// the used slots into per-topic segments [seg_off[k], seg_off[k + 1]); cursor: [K], zero
__global__ __launch_bounds__(256) void phrase_scatter_kernel(const PhraseRec* __restrict__ rec, const u64* __restrict__ slot_rec, const uint32_t* __restrict__ slot_cnt, u64 cap,
                                                             const int64_t* __restrict__ seg_off, u64* cursor, u64* __restrict__ ent_rec, uint32_t* __restrict__ ent_cnt)
{
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cap) return;
    const u64 r = slot_rec[p];
    if (r == SLOT_FREE) return;
    const int32_t k = rec[r].topic;
    const u64 at = (u64)seg_off[k] + atomicAdd(&cursor[k], 1ull);
    ent_rec[at] = r;
    ent_cnt[at] = slot_cnt[p];
}

__device__ __forceinline__ u64 block_sum(u64 v, u64* lds /*[5]*/)   // 256 threads; every thread gets the sum
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & (WV - 1)) == 0) lds[threadIdx.x / WV] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// Block k: cut[k] = the count of topic k's max_n-th most frequent phrase (max_n < 0 or beyond the list: 1, every phrase; max_n = 0: none),
// reach[k] = the phrases with at least that count, occ[k] = the sum of all counts.
__global__ __launch_bounds__(256) void phrase_select_kernel(const int64_t* __restrict__ seg_off, const uint32_t* __restrict__ ent_cnt, int32_t max_n,
                                                            uint32_t* __restrict__ cut, int64_t* __restrict__ reach, int64_t* __restrict__ occ)
{
    __shared__ u64 lds[5];
    const int k = blockIdx.x, t = threadIdx.x;
    const int64_t b = seg_off[k], e = seg_off[k + 1], size = e - b;
    u64 sum = 0, top = 0;
    for (int64_t i = b + t; i < e; i += 256) { const u64 c = ent_cnt[i]; sum += c; top |= c; }
    sum = block_sum(sum, lds);
    for (int o = 32; o > 0; o >>= 1) top |= __shfl_xor(top, o);
    __syncthreads();
    if ((t & (WV - 1)) == 0) lds[t / WV] = top;
    __syncthreads();
    top = lds[0] | lds[1] | lds[2] | lds[3];                   // every bit any count has
    uint32_t c = 1;
    int64_t m = size;
    if (max_n == 0) { c = 0xffffffffu; m = 0; }
    else if (max_n > 0 && (int64_t)max_n < size) {
        c = 0;                                                 // the largest c that at least max_n counts reach
        for (int bit = 63 - __clzll((long long)(top | 1)); bit >= 0; bit--) {
            const uint32_t trial = c | (1u << bit);
            u64 n = 0;
            for (int64_t i = b + t; i < e; i += 256) n += ent_cnt[i] >= trial ? 1 : 0;
            n = block_sum(n, lds);
            if (n >= (u64)max_n) c = trial;
        }
        u64 n = 0;
        for (int64_t i = b + t; i < e; i += 256) n += ent_cnt[i] >= c ? 1 : 0;
        m = (int64_t)block_sum(n, lds);
    }
    if (t == 0) { cut[k] = c; reach[k] = m; occ[k] = (int64_t)sum; }
}

// Block k: the phrases of topic k that reach cut[k], to cand_*[cand_off[k] ..) in no particular order.
__global__ __launch_bounds__(256) void phrase_pack_kernel(const PhraseRec* __restrict__ rec, const int64_t* __restrict__ seg_off, const u64* __restrict__ ent_rec,
                                                          const uint32_t* __restrict__ ent_cnt, const uint32_t* __restrict__ cut, const int64_t* __restrict__ cand_off,
                                                          int64_t* __restrict__ cand_start, int32_t* __restrict__ cand_len, int32_t* __restrict__ cand_cnt)
{
    __shared__ u64 cursor;
    const int k = blockIdx.x, t = threadIdx.x;
    const int64_t b = seg_off[k], e = seg_off[k + 1], room = cand_off[k + 1] - cand_off[k];
    if (room == 0) return;
    if (t == 0) cursor = 0;
    __syncthreads();
    const uint32_t c = cut[k];
    for (int64_t i = b + t; i < e; i += 256) {
        if (ent_cnt[i] < c) continue;
        const u64 at = atomicAdd(&cursor, 1ull);
        if ((int64_t)at >= room) continue;                     // (cannot happen: reach[k] counted the same entries)
        const PhraseRec r = rec[ent_rec[i]];
        const int64_t o = cand_off[k] + (int64_t)at;
        cand_start[o] = r.start; cand_len[o] = r.len; cand_cnt[o] = (int32_t)ent_cnt[i];
    }
}

__global__ __launch_bounds__(256) void phrase_words_kernel(const int32_t* __restrict__ tok, const int64_t* __restrict__ cand_start, const int64_t* __restrict__ word_off, int64_t n,
                                                           int32_t* __restrict__ words)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int64_t s = cand_start[c], o = word_off[c], len = word_off[c + 1] - o;
    for (int64_t i = 0; i < len; i++) words[o + i] = tok[s + i];
}

unsigned blocks_for(u64 n) { return (unsigned)((n + 255) / 256); }

} // namespace

extern "C" int mvhdp_topic_phrases(mvhdp_handle h, const mvhdp_phrase_args* a, int64_t cap_phrases, int64_t cap_words,
                                   int64_t* topic_off, int64_t* word_off, int32_t* words, int32_t* counts, int64_t* distinct, int64_t* occurrences,
                                   int64_t* n_phrases, int64_t* n_words, mvhdp_phrase_stats* stats)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (!a || !n_phrases || !n_words || cap_phrases < 0 || cap_words < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_phrases: null argument or negative cap");
    if (a->hash_bits < 0 || a->hash_bits > 63) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_phrases: hash_bits outside 0..63");
    if (cap_phrases > 0 && (!word_off || !counts)) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_phrases: cap_phrases > 0 with a null output");
    if (cap_words > 0 && !words) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_phrases: cap_words > 0 with null words");
    const bool size_only = cap_phrases == 0 && cap_words == 0 && !word_off && !words && !counts;
    if (!h->have_corpus[0]) FAIL(h, MVHDP_ERR_STATE, "topic_phrases: no view-0 corpus (set_corpus)");
    HIPC(h, hipSetDevice(h->device));
    const int64_t D = mm.D;
    const int32_t* tok = mm.tok[0];
    const u64 hash_mask = a->hash_bits == 0 ? ~0ull : (1ull << a->hash_bits) - 1ull;
    mvhdp_phrase_stats st{};

    // ---- the walk, twice: sizes and validation, then the records ----
    DevArray<u64> ctl, wave_room;
    DevArray<PhraseRec> rec;
    HIPC(h, ctl.alloc(PH_WORDS));
    HIPC(h, ctl.fill(0, h->stream));
    const unsigned walk_blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((D + 3) / 4, (int64_t)h->num_cus * 8));
    const size_t walk_waves = (size_t)walk_blocks * (256 / WV);
    std::vector<u64> room(walk_waves + 1, 0);                  // per wave of the walk's grid: its occurrences, then where its records start
    u64 hc[PH_WORDS] = {};
    HIPC(h, wave_room.alloc(walk_waves));
    if (D > 0) {
        LAUNCH(h, phrase_walk_kernel<false>, dim3(walk_blocks), dim3(256), 0, h->stream, mm.doc_off[0], tok, mm.z[0], D, K, mm.V[0], ctl, wave_room, (PhraseRec*)nullptr, (u64)0);
        HIPC(h, ctl.download(hc, PH_WORDS, h->stream));
        HIPC(h, wave_room.download(room.data(), walk_waves, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    if (hc[PH_BAD]) FAIL(h, MVHDP_ERR_STATE, "topic_phrases: a view-0 token is unassigned (set_assignments), or its topic or its type is out of range");
    u64 n_occ = 0;
    for (size_t q = 0; q < walk_waves; q++) { const u64 c = room[q]; room[q] = n_occ; n_occ += c; }
    st.runs = (int64_t)hc[PH_RUNS];
    st.occurrences = (int64_t)n_occ;

    std::vector<int64_t> h_distinct((size_t)K, 0), h_occ((size_t)K, 0), h_reach((size_t)K, 0), seg_off((size_t)K + 1, 0), cand_off((size_t)K + 1, 0);
    std::vector<int32_t> c_len, c_cnt, c_words;
    std::vector<int64_t> c_woff(1, 0);
    if (n_occ > 0) {
        HIPC(h, rec.alloc((size_t)n_occ));
        HIPC(h, rec.fill(0, h->stream));
        HIPC(h, wave_room.upload(room.data(), walk_waves, h->stream));
        LAUNCH(h, phrase_walk_kernel<true>, dim3(walk_blocks), dim3(256), 0, h->stream, mm.doc_off[0], tok, mm.z[0], D, K, mm.V[0], ctl, wave_room, rec, n_occ);

        // ---- the count by key ----
        u64 cap = 64;
        while (cap < 2 * n_occ) cap <<= 1;
        DevArray<u64> slot_rec, d_distinct, cursor, ent_rec;
        DevArray<uint32_t> slot_cnt, ent_cnt, d_cut;
        DevArray<int64_t> d_seg, d_reach, d_occ;
        HIPC(h, slot_rec.alloc((size_t)cap));
        HIPC(h, slot_cnt.alloc((size_t)cap));
        HIPC(h, d_distinct.alloc((size_t)K));
        HIPC(h, slot_rec.fill(0xff, h->stream));
        HIPC(h, slot_cnt.fill(0, h->stream));
        HIPC(h, d_distinct.fill(0, h->stream));
        LAUNCH(h, phrase_insert_kernel, dim3(blocks_for(n_occ)), dim3(256), 0, h->stream, rec, n_occ, tok, hash_mask, slot_rec, slot_cnt, cap - 1, d_distinct, ctl);
        HIPC(h, d_distinct.download((u64*)h_distinct.data(), (size_t)K, h->stream));   // counts: the same bits either way
        HIPC(h, ctl.download(hc, PH_WORDS, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        st.hash_collisions = (int64_t)hc[PH_COLLISIONS];
        for (int k = 0; k < K; k++) seg_off[(size_t)k + 1] = seg_off[(size_t)k] + h_distinct[(size_t)k];
        const int64_t n_distinct = seg_off[(size_t)K];
        st.distinct = n_distinct;

        // ---- per topic: the cut, and who reaches it ----
        HIPC(h, d_seg.alloc((size_t)K + 1));
        HIPC(h, cursor.alloc((size_t)K));
        HIPC(h, ent_rec.alloc((size_t)n_distinct));
        HIPC(h, ent_cnt.alloc((size_t)n_distinct));
        HIPC(h, d_cut.alloc((size_t)K));
        HIPC(h, d_reach.alloc((size_t)K));
        HIPC(h, d_occ.alloc((size_t)K));
        HIPC(h, d_seg.upload(seg_off.data(), (size_t)K + 1, h->stream));
        HIPC(h, cursor.fill(0, h->stream));
        LAUNCH(h, phrase_scatter_kernel, dim3(blocks_for(cap)), dim3(256), 0, h->stream, rec, slot_rec, slot_cnt, cap, d_seg, cursor, ent_rec, ent_cnt);
        LAUNCH(h, phrase_select_kernel, dim3((unsigned)K), dim3(256), 0, h->stream, d_seg, ent_cnt, a->max_per_topic, d_cut, d_reach, d_occ);
        HIPC(h, d_reach.download(h_reach.data(), (size_t)K, h->stream));
        HIPC(h, d_occ.download(h_occ.data(), (size_t)K, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        for (int k = 0; k < K; k++) cand_off[(size_t)k + 1] = cand_off[(size_t)k] + h_reach[(size_t)k];
        const int64_t n_cand = cand_off[(size_t)K];

        // ---- what crosses: the kept phrases and the count ties at the cut ----
        if (n_cand > 0) {
            DevArray<int64_t> d_coff, c_start, d_woff;
            DevArray<int32_t> d_len, d_cnt, d_words;
            HIPC(h, d_coff.alloc((size_t)K + 1));
            HIPC(h, c_start.alloc((size_t)n_cand));
            HIPC(h, d_len.alloc((size_t)n_cand));
            HIPC(h, d_cnt.alloc((size_t)n_cand));
            HIPC(h, d_coff.upload(cand_off.data(), (size_t)K + 1, h->stream));
            LAUNCH(h, phrase_pack_kernel, dim3((unsigned)K), dim3(256), 0, h->stream, rec, d_seg, ent_rec, ent_cnt, d_cut, d_coff, c_start, d_len, d_cnt);
            c_len.resize((size_t)n_cand); c_cnt.resize((size_t)n_cand);
            HIPC(h, d_len.download(c_len.data(), (size_t)n_cand, h->stream));
            HIPC(h, d_cnt.download(c_cnt.data(), (size_t)n_cand, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
            c_woff.resize((size_t)n_cand + 1);
            for (int64_t c = 0; c < n_cand; c++) c_woff[(size_t)c + 1] = c_woff[(size_t)c] + c_len[(size_t)c];
            const int64_t nw = c_woff[(size_t)n_cand];
            HIPC(h, d_woff.alloc((size_t)n_cand + 1));
            HIPC(h, d_words.alloc((size_t)nw));
            HIPC(h, d_woff.upload(c_woff.data(), (size_t)n_cand + 1, h->stream));
            LAUNCH(h, phrase_words_kernel, dim3(blocks_for((u64)n_cand)), dim3(256), 0, h->stream, tok, c_start, d_woff, n_cand, d_words);
            c_words.resize((size_t)nw);
            HIPC(h, d_words.download(c_words.data(), (size_t)nw, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
        }
    }

    // ---- the order inside equal counts, and the cut ----
    std::vector<int64_t> order, t_off((size_t)K + 1, 0);
    int64_t total_words = 0;
    for (int k = 0; k < K; k++) {
        const int64_t c0 = cand_off[(size_t)k], c1 = cand_off[(size_t)k + 1];
        std::vector<int64_t> idx((size_t)(c1 - c0));
        for (int64_t c = c0; c < c1; c++) idx[(size_t)(c - c0)] = c;
        std::sort(idx.begin(), idx.end(), [&](int64_t l, int64_t r) {
            if (c_cnt[(size_t)l] != c_cnt[(size_t)r]) return c_cnt[(size_t)l] > c_cnt[(size_t)r];
            return std::lexicographical_compare(c_words.begin() + c_woff[(size_t)l], c_words.begin() + c_woff[(size_t)l + 1],
                                                c_words.begin() + c_woff[(size_t)r], c_words.begin() + c_woff[(size_t)r + 1]);
        });
        int64_t keep = h_distinct[(size_t)k];
        if (a->max_per_topic >= 0 && keep > a->max_per_topic) keep = a->max_per_topic;
        if (keep > c1 - c0) FAIL(h, MVHDP_ERR_HIP, "topic_phrases: fewer candidates than phrases to keep");
        for (int64_t q = 0; q < keep; q++) { order.push_back(idx[(size_t)q]); total_words += c_len[(size_t)idx[(size_t)q]]; }
        t_off[(size_t)k + 1] = t_off[(size_t)k] + keep;
    }
    const int64_t kept = (int64_t)order.size();
    st.kept = kept;
    *n_phrases = kept;
    *n_words = total_words;
    if (!size_only && (kept > cap_phrases || total_words > cap_words)) FAIL(h, MVHDP_ERR_INVALID_ARG, "topic_phrases: more phrases or words than cap (the sizes are set)");
    if (topic_off) memcpy(topic_off, t_off.data(), t_off.size() * sizeof(int64_t));
    if (distinct) memcpy(distinct, h_distinct.data(), (size_t)K * sizeof(int64_t));
    if (occurrences) memcpy(occurrences, h_occ.data(), (size_t)K * sizeof(int64_t));
    if (stats) *stats = st;
    if (size_only) return MVHDP_OK;
    int64_t wo = 0;
    if (word_off) word_off[0] = 0;
    for (int64_t q = 0; q < kept; q++) {
        const int64_t c = order[(size_t)q];
        counts[q] = c_cnt[(size_t)c];
        for (int64_t i = c_woff[(size_t)c]; i < c_woff[(size_t)c + 1]; i++) words[wo++] = c_words[(size_t)i];
        word_off[q + 1] = wo;
    }
    return MVHDP_OK;
}
