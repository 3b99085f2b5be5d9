/*
 * mvhdp.h — C ABI of libmvhdp.so: the MI355X (gfx950) multi-view HDP
 * collapsed-Gibbs sweep that replaces the iteration body of
 * FastQMVWVParallelTopicModel.estimate() in hmetaxa/MVTopicModel.
 *
 * Reference aliases (under src/main/java/org/madgik/ of the reference):
 *   PTM = MVTopicModel/FastQMVWVParallelTopicModel.java
 *   WRK = MVTopicModel/FastQMVWVWorkerRunnable.java
 *   UPD = MVTopicModel/FastQMVWVUpdaterRunnable.java
 *   FT  = utils/FTree.java   QD = utils/FastQDelta.java
 *   MTA = utils/MixTopicModelTopicAssignment.java
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns
 * 0 (MVHDP_OK) or a negative mvhdp_status; no exceptions cross the boundary;
 * the caller owns every host buffer, the library copies.  A handle is bound to
 * one HIP device and is not thread-safe (estimate() is single-threaded,
 * PTM:1033).  The JNI stub that binds these entry points from Java is shown
 * in INTEGRATION.md.
 */
#ifndef MVHDP_H
#define MVHDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVHDP_MAX_MODALITIES 8
#define MVHDP_MAX_TOPICS     2048
#define MVHDP_UNASSIGNED_TOPIC (-1)          /* PTM:63 */

typedef enum {
    MVHDP_OK = 0,
    MVHDP_ERR_INVALID_ARG   = -1,
    MVHDP_ERR_STATE         = -2,  /* call order violated (e.g. sweep before set_corpus) */
    MVHDP_ERR_HIP           = -3,  /* HIP runtime failure, see mvhdp_last_error */
    MVHDP_ERR_NO_DEVICE     = -4,  /* no gfx950 device: there is NO CPU fallback */
    MVHDP_ERR_NEGATIVE_COUNT= -5,  /* a count went below zero (the reference only logs it, UPD:202-215) */
    MVHDP_ERR_UNSUPPORTED   = -6
} mvhdp_status;

typedef struct mvhdp_ctx* mvhdp_handle;

/* Shape of the model: replaces the ctor arguments PTM:183 + numTypes PTM:413. */
typedef struct {
    int32_t num_topics;                          /* K, PTM:193 */
    int32_t num_modalities;                      /* M, PTM:189 */
    int32_t num_types[MVHDP_MAX_MODALITIES];     /* V_m = alphabet[m].size(), PTM:413; below 2^29 (two bits of a type id carry the row's class inside the kernels) */
    int32_t device;                              /* HIP device ordinal */
    int64_t doc_id_base;                         /* global id of local entity 0 (document shards, one per GPU) */
    uint32_t flags;                              /* reserved, 0 */
} mvhdp_config;

/* Hyper-parameters the sampler reads: PTM:79-83,130-131,95. */
typedef struct {
    const double* alpha;                         /* [M][K+1], index K = new-topic weight PTM:196 */
    double alpha_sum[MVHDP_MAX_MODALITIES];      /* PTM:80 */
    double beta[MVHDP_MAX_MODALITIES];           /* PTM:81 */
    double beta_sum[MVHDP_MAX_MODALITIES];       /* PTM:82, = beta*V_m PTM:420 */
    double gamma[MVHDP_MAX_MODALITIES];          /* PTM:83 */
    double p_a[MVHDP_MAX_MODALITIES][MVHDP_MAX_MODALITIES]; /* PTM:130 */
    double p_b[MVHDP_MAX_MODALITIES][MVHDP_MAX_MODALITIES]; /* PTM:131 */
    const uint8_t* inactive;                     /* [K] 1 = member of inActiveTopicIndex (PTM:95); NULL = none */
} mvhdp_hyper;

/* What one sweep reports: the reference's branch counters WRK:33-35 plus
 * bookkeeping. */
typedef struct {
    int64_t tokens;               /* tokens sampled */
    int64_t changed;              /* tokens whose topic changed = FastQDelta records, WRK:587 */
    int64_t new_mass_cnt;         /* WRK:523 */
    int64_t topic_doc_mass_cnt;   /* WRK:530 */
    int64_t word_ftree_mass_cnt;  /* WRK:533 */
    int64_t oov_skipped;          /* WRK:427-428 */
    int64_t aborted_docs;         /* Q11 (WRK:599-601): always 0 unless a mass is NaN */
    int64_t exact_fallbacks;      /* tokens that left the certified scan for the sequential sum */
    int32_t activated_topic;      /* UPD:263-270: topic leaving inActiveTopicIndex, -1 if none */
    int32_t activated_modality;   /*   and the view whose alpha[m][k] took alpha[m][K] */
    int64_t activation_key;       /* ordering key of that first delta, MVHDP_ACT_KEY(doc, view, pos, topic); INT64_MAX if none */
    double  sweep_kernel_ms;      /* device time of the sweep kernel alone (hipEvents on the handle's stream) */
    double  total_ms;             /* device time of the whole call: trees + view weights + sweep + apply */
    int32_t activations;          /* topics that left inActiveTopicIndex during this call: 0 or 1 for a deferred sweep; a SEGMENT_APPLY sweep or a
                                     LIVE sweep on stored trees activates one per segment border (up to its segment count); a LIVE sweep in its
                                     live-rows form gives birth chunk by chunk (any number: see MVHDP_SWEEP_LIVE); activated_topic is the FIRST of them
                                     -- a host pulls alpha / inActiveTopicIndex with mvhdp_get_alpha whenever activated_topic >= 0;
                                     0 with MVHDP_SWEEP_NO_APPLY / FROZEN (the caller activates: mvhdp_apply_delta, or mvhdp_activate_births
                                     behind a MVHDP_SWEEP_SHARD_BIRTHS sweep); a group sweep reports what it activated on every member:
                                     with SHARD_BIRTHS the number of topics born in the step, activated_topic the lowest-index newborn */
    int32_t reserved;
} mvhdp_sweep_stats;

/* Activation key: the FastQDelta that activates a topic first in (global entity, view, position) order wins (UPD:263-270
 * with a single updater).  One definition for the kernels, the host and any binding (multi-GPU: MIN-all-reduce the key). */
#define MVHDP_ACT_DOC_SHIFT   34
#define MVHDP_ACT_VIEW_SHIFT  31
#define MVHDP_ACT_POS_SHIFT   11
#define MVHDP_ACT_TOPIC_MASK  0x7ffLL
#define MVHDP_ACT_VIEW_MASK   0x7LL
#define MVHDP_ACT_KEY(doc, view, pos, topic) \
    (((int64_t)(doc) << MVHDP_ACT_DOC_SHIFT) | ((int64_t)(view) << MVHDP_ACT_VIEW_SHIFT) | ((int64_t)(pos) << MVHDP_ACT_POS_SHIFT) | (int64_t)(topic))
#define MVHDP_ACT_KEY_TOPIC(key) ((int32_t)((key) & MVHDP_ACT_TOPIC_MASK))
#define MVHDP_ACT_KEY_VIEW(key)  ((int32_t)(((key) >> MVHDP_ACT_VIEW_SHIFT) & MVHDP_ACT_VIEW_MASK))
#define MVHDP_ACT_KEY_NONE INT64_MAX

/* Optional debug outputs of a sweep (parity tests only; slows the kernel). */
typedef struct {
    /* per view: 4 doubles per token {newTopicMass, topicDocWordMass, tree root, sample}
     * (WRK:515-519); NULL entries are skipped. Host pointers. */
    double* tok_dbg[MVHDP_MAX_MODALITIES];
    /* full conditionals of selected tokens: (doc, view, pos) -> K+1 doubles,
     * normalised; slot K is the new-topic mass (SURVEY §8a "full conditional"). */
    int32_t n_trace;
    const int64_t* trace_doc;     /* local entity index */
    const int32_t* trace_view;
    const int32_t* trace_pos;
    double* trace_out;            /* [n_trace][K+1] host */
} mvhdp_debug;

/* sweep flags */
#define MVHDP_SWEEP_REUSE_TREES 0x1u  /* do not rebuild the F+trees from the counts first (PTM:1209 cadence is the host's) */
#define MVHDP_SWEEP_NO_APPLY    0x2u  /* leave the deltas unapplied (multi-GPU: all-reduce MVHDP_BUF_DELTA, then mvhdp_apply_delta).
                                       * The delta buffer may be written by the caller only between such a sweep and mvhdp_apply_delta. */
#define MVHDP_SWEEP_EXACT_CHAIN 0x4u  /* always use the sequential WRK:501-513 sum (test mode for the certified scan) */
#define MVHDP_SWEEP_GENERIC_KERNEL 0x8u /* force the LDS-resident kernel even when the register-resident one applies (test mode) */
#define MVHDP_SWEEP_FROZEN      0x10u /* the inferencer's call of the same worker (INF:211-294: nst=1, nut=0): sample against the
                                         stored trees and counts, queue no deltas (WRK:587), leave the model untouched */

/* The reference's own update discipline (UPD:197-218 applied WHILE the workers sample; PTM:84-87: racy reads by design):
 * the sweep's n_wk atomics go straight to the shared count array and every later token of the sweep reads them.  Not
 * reproducible run to run (like the reference); counts stay consistent with z.  The entities are cut into
 * MVHDP_SWEEP_LIVE_SEGMENTS(n) interleaved segments (n = 1..255, 0 = library default); at each segment boundary the
 * tokensPerTopic updates of the segment (privatised per workgroup: M*K hot words) land.
 * The tree branch (WRK:533-535) -- two forms, mvhdp_tuning.live_rows:
 *   live rows (default wherever every kernel of the sweep is register-resident; default 1 segment): no stored tree is sampled for a
 *     word of at most 65534 tokens; the branch draws from leaf_k = coef_k * (n_wk + beta) with n_wk the word's LIVE row, read when the
 *     token's turn comes, and coef_k = gamma alpha_k / (n_k + beta Sigma) of the segment start -- what the reference's updater achieves
 *     by refreshing the two touched leaves with every delta (UPD:242-260 -> FT:138-147).  Heavier words keep stored trees, rebuilt from
 *     the live counts over and over by a kernel that runs beside the samplers;
 *   stored trees (live_rows = 0, and wherever the generic kernel serves: default 4 segments): the F+trees are rebuilt from the live
 *     counts at every segment boundary (with REUSE_TREES: no rebuild at all, the host's PTM:1209 cadence).
 * With NO_APPLY the delta buffer receives (counts after - counts before) of this shard and counts are restored, so the
 * multi-GPU sequence all-reduce + mvhdp_apply_delta is the same as for a deferred sweep.  Not combinable with FROZEN.
 * (LIVE_SEGMENTS without LIVE cuts a deferred sweep into the same segments: same integers as one segment.)
 * Topic activation (UPD:263-270): the first delta of a SEGMENT that lands on an inactive topic activates it at the segment's
 * end -- alpha[m][k] takes alpha[m][K], the topic leaves inActiveTopicIndex, the next segment's new-topic draws go to the
 * next inactive index (WRK:523-526) -- so one sweep can give birth to up to n topics (mvhdp_sweep_stats.activations); the
 * reference's updater does it delta by delta (on C5 its 100 inactive topics are all born within the first sweep).  A live sweep in
 * its live-rows form does it chunk by chunk: a new-topic draw takes the first inactive topic no delta has reached yet, a chunk whose
 * deltas reach it moves the samplers on to the next, and the segment's end activates every topic that was reached, in index order
 * (mvhdp_sweep_stats.activations can exceed the segment count).  With NO_APPLY nothing is activated here (the caller reduces the
 * key first) and new-topic draws all go to the first inactive index -- unless MVHDP_SWEEP_SHARD_BIRTHS asks for the births of a
 * document shard (below). */
#define MVHDP_SWEEP_LIVE        0x20u
#define MVHDP_SWEEP_LIVE_SEGMENTS(n) (((uint32_t)(n) & 0xffu) << 16)

/* A deferred sweep cut into MVHDP_SWEEP_LIVE_SEGMENTS(n) segments WITH the updater catching up in between: every
 * segment is a snapshot sweep over its entities (trees rebuilt from the current counts, deltas collected), then its deltas
 * are applied before the next segment starts.  Bit-reproducible like the plain deferred sweep (the oracle follows it
 * segment by segment), and statistically between the deferred and the live sweep: a token sees counts that are at most
 * one segment old.  Single handle only (not combinable with NO_APPLY, LIVE or FROZEN); a topic is activated at the end of
 * the segment whose delta reached it first (as for LIVE above).  The segments are the interleaved ones of the live sweep: positions s, s+n, s+2n, ... of the
 * entities ordered by decreasing token count (ties by entity index). */
#define MVHDP_SWEEP_SEGMENT_APPLY 0x40u

/* With MVHDP_SWEEP_SEGMENT_APPLY: the updater runs BESIDE the samplers, as UPD:164-297 runs beside WRK:186-233 -- the deltas of
 * segment s are applied to the counts while segment s+1 is being sampled, so segment s+2 is the first to see them: every token of
 * segment s samples against the counts after segment s-2 (segments 0 and 1: the sweep-start counts).  The F+trees are built once, at
 * the start of the sweep, and serve every segment: a DEVIATION from the reference, whose updater refreshes the two touched leaves with
 * every delta (UPD:242-260) so that its trees follow the counts -- here a token's tree-branch mass and its count-based branch come from
 * different model states (plain SEGMENT_APPLY rebuilds the trees at every segment border).  Still a deterministic chain,
 * followed by the oracle segment by segment (tests/test_gpu_segmented.py); and without the per-segment stall of plain SEGMENT_APPLY:
 * two segments are in flight, no kernel boundary idles the chip (the counts and their mirror are kept twice).  Not with inactive
 * topics (the activation of UPD:263-270 needs the host between segments): MVHDP_ERR_UNSUPPORTED. */
#define MVHDP_SWEEP_SEGMENT_OVERLAP 0x80u

/* Only segment s (0-based) of the MVHDP_SWEEP_LIVE_SEGMENTS(n) interleaved segments is swept: the entities at positions s, s+n,
 * s+2n, ... of the longest-first order; the statistics cover those entities.  With it a HOST drives a segmented sweep and can put
 * anything between two segments -- an all-reduce over document shards, a look at the counts (tests/test_gpu_full_size.py checks
 * every segment of a full-size segmented sweep against the oracle this way).  n calls with s = 0..n-1 of a deferred sweep (each
 * applying its deltas) give the integers of one MVHDP_SWEEP_SEGMENT_APPLY call with n segments.  Not with LIVE or SEGMENT_APPLY. */
#define MVHDP_SWEEP_ONLY_SEGMENT(s) ((((uint32_t)(s) + 1u) & 0xffu) << 24)

/* Births of a truncated HDP on a document shard (UPD:263-270, WRK:522-526).  Only with MVHDP_SWEEP_LIVE; MVHDP_ERR_INVALID_ARG
 * without it, with FROZEN, and with ONLY_SEGMENT.  With NO_APPLY, over a model with inactive topics, in the live-rows form: the
 * sweep gives birth chunk by chunk as a live sweep without NO_APPLY does (one list of the inactive topics for the whole call: nothing
 * restarts at a segment border) but activates nothing -- a topic it reached keeps its zero coefficient until the caller activates it.
 * Without NO_APPLY, or without inactive topics, the flag changes nothing.  Every shard starts from the same replicated list and only
 * moves forward along it, so what each reaches is a prefix of the list and so is the union over the shards: the caller MIN-reduces
 * the per-topic table MVHDP_BUF_BIRTH_KEYS over all shards (RCCL ncclMin over K int64, in place) and every replica calls
 * mvhdp_activate_births with the result.  In the stored-tree form (mvhdp_tuning.live_rows = 0, or wherever the generic kernel
 * serves) topics are not born chunk by chunk: the table then holds at most the sweep's activation key, at its own topic.
 * mvhdp_group_sweep takes the flag with LIVE (the same on every rank, as every flag): the K-wide MIN-reduce replaces the 8-byte
 * one, and a step activates every topic any shard reached. */
#define MVHDP_SWEEP_SHARD_BIRTHS 0x200u

/* device buffers a host may hand to a collective (RCCL through torch.distributed or directly) */
typedef enum {
    MVHDP_BUF_COUNTS = 0,  /* int32 [sumV*K + M*K]: n_wk rows of every view, then n_k */
    MVHDP_BUF_DELTA  = 1,  /* int32 [sumV*K + M*K]: the last sweep's deltas, same layout */
    MVHDP_BUF_BIRTH_KEYS = 2, /* int64 [K]: written by every NO_APPLY sweep: keys[k] = the first delta (MVHDP_ACT_KEY) that reached topic k
                                 if k was inactive and was reached, MVHDP_ACT_KEY_NONE otherwise (see MVHDP_SWEEP_SHARD_BIRTHS) */
    /* read-only views for tests and diagnostics, not for collectives: what the last tree build left (deferred sweeps gather from them).
       UNSTABLE: the packed layout and the class bits are internals of the sweep kernels and may change with any release; a host must not
       build on them. */
    MVHDP_BUF_COUNTS12 = 3,   /* bytes [sumV][128 * ceil(K / 85)]: the 12-bit image of n_wk, a row valid where its class says so (DESIGN.md
                                 section 3); MVHDP_ERR_INVALID_ARG on a handle that keeps none (short rows, a view of 2^28 types or more) */
    MVHDP_BUF_ROW_CLASS = 4   /* bytes [sumV]: bits 1:0 the row's weight class (0 small, 1 heavy, 2 big), bit 2: the row is in the 12-bit image */
} mvhdp_buffer;

/* ---- lifetime ---- */
int mvhdp_create(const mvhdp_config* cfg, mvhdp_handle* out);   /* replaces new FastQMVWV…TopicModel PTM:183 + initSpace PTM:575 */
int mvhdp_destroy(mvhdp_handle h);
const char* mvhdp_last_error(mvhdp_handle h);                    /* h may be NULL: last create error */
const char* mvhdp_version(void);

/* ---- corpus and assignments: MTA / MALLET FeatureSequence + LabelSequence flattened to CSR ---- */
/* One call per view m; D entities in `data` order (PTM:443-455); an entity
 * without view m (Assignments[m]==null, MTA:19) is an empty span. */
int mvhdp_set_corpus(mvhdp_handle h, int32_t m, int64_t num_docs,
                     const int64_t* doc_off /*[D+1]*/, const int32_t* tokens /*[N_m]*/);
int mvhdp_set_assignments(mvhdp_handle h, int32_t m, const int32_t* z /*[N_m]*/);  /* topicSequence.getFeatures() PTM:481 */
/* Which entities HAVE view m (Assignments[m] != null, MTA:19): present[d] = 1 also for an instance with an empty FeatureSequence,
 * which the CSR alone cannot tell from a missing one.  NULL (the default) = present iff the span is non-empty.  The sweep does not
 * care (WRK:341,403 treat null and length 0 alike); the statistics do: modelLogLikelihood's two phantom tokens of topic 0 and its
 * modalityCnt (PTM:3348-3373: the backing array of an empty LabelSequence has length 2), totalDocsPerModality and
 * docLengthCounts[0] (PTM:620-651), and the carry-over of printDocumentTopics (PTM:2873-2886: a present empty view scores with
 * zeros, a missing one with the previous holder's counts).  Call after mvhdp_set_corpus of that view. */
int mvhdp_set_view_presence(mvhdp_handle h, int32_t m, const uint8_t* present /*[D] or NULL*/);
int mvhdp_get_assignments(mvhdp_handle h, int32_t m, int32_t* z /*[N_m]*/);

/* ---- model state ---- */
int mvhdp_set_hyper(mvhdp_handle h, const mvhdp_hyper* hy);
int mvhdp_get_alpha(mvhdp_handle h, double* alpha /*[M][K+1]*/, uint8_t* inactive /*[K]*/); /* after a topic activation UPD:263-270 */
int mvhdp_build_counts(mvhdp_handle h);                          /* buildInitialTypeTopicCounts PTM:600-652 */
int mvhdp_build_trees(mvhdp_handle h);                           /* buildFTrees PTM:2660-2696 */
int mvhdp_build_inference_trees(mvhdp_handle h);                 /* FastQMVWVTopicInferencer.initInferencer INF:557-586: leaves p_wt, no gamma*alpha */
/* INF:169-199: z = trees[m][type].sample(u) for in-vocabulary tokens, 0 otherwise; u from the token stream with sweep 0xFFFFFFFF */
int mvhdp_init_assignments_from_trees(mvhdp_handle h, uint64_t seed);
int mvhdp_get_counts(mvhdp_handle h, int32_t m, int32_t* n_wk /*[V_m][K] or NULL*/, int32_t* n_k /*[K] or NULL*/);
int mvhdp_set_counts(mvhdp_handle h, int32_t m, const int32_t* n_wk, const int32_t* n_k);
int mvhdp_get_tree(mvhdp_handle h, int32_t m, int32_t type, double* tree /*[2K], FTree.tree FT:21*/);
/* topicDocCounts[m][k][c] (c < hist_len) and docLengthCounts[m][len] (PTM:107-108,
 * 620-651), recomputed from z instead of the updater's incremental bookkeeping
 * UPD:220-232. Either output may be NULL. */
int mvhdp_get_doc_topic_hist(mvhdp_handle h, int32_t m, int32_t* hist /*[K][hist_len]*/, int32_t hist_len,
                             int32_t* doc_len_counts /*[len_len]*/, int32_t len_len);

/* ---- the steps either side of the sweep: statistics the host's optimize* and logging need ---- */
/* countHistogram of optimizeBeta PTM:2295-2309: hist[c] = number of (type, topic) pairs of view m holding count c (c >= 1, c < len). */
int mvhdp_get_count_histogram(mvhdp_handle h, int32_t m, int32_t* hist, int32_t len);
/* optimizeP PTM:2706-2792: sums[m][i] = sum over entities, in entity order, of pDistr_Mean[m][i][doc]. */
int mvhdp_view_overlap_sums(mvhdp_handle h, double* sums /*[M][M]*/);
/* modelLogLikelihood PTM:3322-3452, one value per view. */
int mvhdp_model_log_likelihood(mvhdp_handle h, double* log_likelihood /*[M]*/);
/* optimizeGamma PTM:2415-2433, the document level (Teh et al. 2006): over the entities that have view m, of length j,
 * qs = sum Bernoulli(j/(j+gamma_m)) and qw = sum log Beta(gamma_m+1, j).  The reference draws them sequentially from a
 * stream that cannot be seeded (RandomSamplers over ThreadLocalRandom, PTM:236), ten rounds per view; here every entity
 * draws from its own counter-based stream (seed, global entity id, view, round): the same random variables in distribution,
 * reproducible, shard-independent.  A host keeps its closed-form updates and calls this for the two sums. */
int mvhdp_gamma_doc_statistics(mvhdp_handle h, int32_t m, double gamma_m, uint64_t seed, uint32_t round, double* qs, double* qw);
/* optimizeDP PTM:2454-2488, the view-table simulation over topicDocCounts[m] (hist [K][hist_len] as mvhdp_get_doc_topic_hist or
 * mvhdp_group_doc_topic_hist returns it: host memory).  For every cell (topic t, count i) that holds entities: i == 1 adds them; i > 1
 * adds them times ONE draw of the number of tables a CRP(conc[t]) makes of i items (conc[t] = gamma[m] * alpha[m][t], PTM:2471) -- the
 * Antoniak distribution, drawn as the sum of the i - 1 Bernoulli(conc / (conc + l)) table openings from a counter-based stream
 * (seed, round, view, topic, count).  The reference draws it through a table of Stirling numbers from a stream that cannot be seeded
 * and scales the CACHED table row in place on every call (Samplers.java:1086-1110); a host that wants that sequence keeps its own loop
 * (the default of the host classes), one that wants the statistic calls this.  mk[t]: the sum over the cells; active[t]: 1 iff a cell
 * with i >= 1 holds an entity (PTM:2461,2480: the topic leaves inActiveTopicIndex).  The root level (PTM:2491-2517: K * M draws) stays
 * with the host. */
int mvhdp_dp_table_statistics(mvhdp_handle h, int32_t m, const int32_t* hist /*[K][hist_len]*/, int32_t hist_len, const double* conc /*[K]*/,
                              uint64_t seed, uint32_t round, double* mk /*[K]*/, uint8_t* active /*[K]*/);
/* n independent draws of the same kind -- optimizeDP's root level PTM:2491-2517 asks for K * M of them, randAntoniak(gammaRoot,
 * ceil(mk[m][t])): tables[j] = the number of tables a CRP(conc[j]) makes of items[j] items; items <= 0: 0, 1: 1, more than 20000
 * (the reference's MAXSTIRLING, Samplers.java:1024: its call throws there and PTM:2507-2509 falls back to one table): 1. */
int mvhdp_antoniak_draws(mvhdp_handle h, int32_t n, const int32_t* items /*[n]*/, const double* conc /*[n]*/, uint64_t seed, uint32_t round, int32_t* tables /*[n]*/);
/* printDocumentTopics PTM:2871-2899 (and the inferencer's INF:383-411): topic proportions of entities [d0, d1),
 * out[(d-d0)*K + k] = sum_m w[m]*(n_dk[m][k] + gamma[m]*alpha[m][k])/(len[m] + gamma[m]*alphaSum[m]) / sum_m w[m],
 * w[m] = (m == 0 ? 1 : discrWeightPerModality[m]) * pMean[0][m].  As in the reference, whose topicCounts[m] / docLen[m]
 * are refreshed only when the entity has view m (PTM:2873-2886), an entity WITHOUT view m is scored with n_dk[m] and
 * len[m] of the last earlier entity of this handle that had it (zeros before the first). */
int mvhdp_doc_topic_proportions(mvhdp_handle h, const double* view_weights /*[M]*/, int64_t d0, int64_t d1, double* out /*[d1-d0][K]*/);

/* ---- after training: what SciTopicFlow does with a trained model (FLOW = MVTopicModel/SciTopicFlow.java, FLOW:246-260) ----
 * saveTopicsPerDoc PTM:2821-2926 (the inferencer's printDocumentTopics INF:332-490) -> the thresholded, sorted topic list per entity;
 * CalcEntityTopicDistributionsAndTrends FLOW:807-1083 -> those lists summed per author / project / venue / batch / corpus and normalised;
 * calcSimilarities FLOW:1320-1532 and CalcTopicSimilarities FLOW:1084-1196 -> every pair of the resulting vectors compared. */

/* PTM:2890-2926: the topic list of entities [d0, d1).  The proportions have exactly the bits of mvhdp_doc_topic_proportions (its
 * missing-view carry-over included).  Per entity the topics are ordered as IDSorter.compareTo orders them (mallet-2.0.8 class file):
 * weight descending, equal weights by DESCENDING topic id; the reference sets entry k of its IDSorter array to (k, weight) for every
 * document (PTM:2890-2901), so nothing carries over between documents.  The list is cut at the first weight < threshold (PTM:2911) and
 * at max entries (max < 0 or max > K: K, PTM:2867-2869).  Weights are unrounded (the (double) Math.round(w * 10000) / 10000 of PTM:2919 is
 * the caller's, or mvhdp_entity_topic_distributions').  row_off[d - d0] .. row_off[d - d0 + 1] index topics / weights.
 * Capacity: topics and weights NULL with cap = 0 returns *count (and row_off, unless NULL) only; more than cap entries:
 * MVHDP_ERR_INVALID_ARG, *count set, the arrays untouched.  Preconditions as mvhdp_doc_topic_proportions. */
int mvhdp_doc_topics_top(mvhdp_handle h, const double* view_weights /*[M]*/, int64_t d0, int64_t d1, double threshold, int32_t max,
                         int64_t cap, int64_t* row_off /*[d1-d0+1]*/, int32_t* topics, double* weights, int64_t* count);
/* FLOW:807-1083 on the lists above.  The flow stores floor(w * 10^4 + 0.5) / 10^4 of every kept weight (PTM:2919) and lets SQL sum them
 * per group and divide by the group's total (FLOW:880-1010); an SQL engine's summation order is not reproducible, so THIS definition is
 * ours: for group g, out[g][k] = sum over members[member_off[g] .. member_off[g+1]), in that order, of the rounded kept weight of topic k;
 * the total is one chain over the members in that order and, within a member, its kept topics in ascending topic id; every sum is
 * divided by the total and, unless round_digits is -1, rounded as floor(v * 10^digits + 0.5) / 10^digits (round_digits 0..15; the SQL
 * uses 5).  Fixed order, no floating-point atomics: two calls give the same bits.  A group with total 0 (or no member) is a row of
 * zeros.  members are entity ids of this handle, in any order, repeated across (or within) groups at will. */
int mvhdp_entity_topic_distributions(mvhdp_handle h, const double* view_weights, double threshold, int32_t max, int32_t round_digits /*-1: none*/,
                                     int64_t n_groups, const int64_t* member_off /*[n_groups+1]*/, const int64_t* members /*entity ids, may repeat across groups*/,
                                     double* out /*[n_groups][K]*/);

/* calcSimilarities FLOW:1320-1532 (threshold 0.15) / CalcTopicSimilarities FLOW:1084-1196 (0.3): all pairs i < j of the n rows of x with
 * sim(i, j) > threshold -- strictly, as FLOW:1146,1462,1484 -- sorted by (i, j), sim unrounded (the flow's (double) Math.round(sim * 1000) /
 * 1000, FLOW:1152,1467,1488, is the caller's).  An entry x[r][c] <= min_weight counts as 0 (the NormWeight > 0.03 of the SQL at FLOW:1341;
 * -inf: none).  Entries are expected finite.
 * Cosine metrics, bit for bit the reference's arithmetic (read from mallet-2.0.8's class files): dot = the unfused fp64 chain
 * s = s + a_k * b_k over ascending k (SparseVector.dotProductInternal walks the first vector's locations in ascending index, dmul then
 * dadd; an absent entry is an exact zero product, so the dense chain has the same bits; MatrixOps.dotProduct is the dense loop itself),
 * |a| = Math.sqrt of the same chain of squares (SparseVector.twoNorm, MatrixOps.twoNorm), then dot / (|a| * |b|)
 * (NormalizedDotProductMetric.distance = 1 - that; org.madgik.utils.Utils.cosineSimilarity :18-22), then for COS_FOLDED 1 - |1 - c|.
 * FLOW:1144 takes max(cosine, 0) before its test; with threshold >= 0 that changes no decision and no emitted value.
 * Two stages.  (a) Screen, on the matrix cores: rows normalised in fp64, stored as fp32, multiplied in 128 x 128 tiles (on and above the
 * diagonal only) with v_mfma_f32_32x32x2_f32, an exact k-ordered fp32 fma chain; a pair is a candidate when
 * screen > threshold - margin, margin(dim) = (dim + 4) * 2^-23: the normalised rows have sum |a_k b_k| <= 1, rounding the inputs to fp32
 * moves the sum by at most 2 * 2^-24 of that and a chain of dim fp32 terms by at most dim * 2^-24; the margin is twice the sum of the
 * two.  dim > 65536: MVHDP_ERR_UNSUPPORTED (the margin stays below 0.01).  (b) Exact: every candidate recomputed by the fp64 chain and
 * tested.  The screen never decides a pair.  The bound holds where fp64 neither under- nor overflows: a row with a non-zero |entry|
 * outside [2^-500, 2^500] is not screened at all -- each of its pairs is a candidate.  A row whose norm is 0, Inf or NaN never yields a
 * pair (in Java NaN compares false and 0 is not > threshold >= 0) and is left out of both stages.
 * MVHDP_SIM_JSD: Maths.jensenShannonDivergence (class file): m_k = (p_k + q_k) / 2, (KL(p, m) + KL(q, m)) / 2,
 * KL(p, m) = (sum over ascending k with p_k != 0 of p_k * Math.log(p_k / m_k)) / Math.log(2), +inf when such an m_k is 0.  A plain fp64
 * kernel, no screen; Math.log and the device's log may differ by an ulp, so values agree with Java to a few ulp per term, not bit for
 * bit.  Rows of norm 0 / Inf / NaN are left out as above.
 * What the reference does differently, and we do not follow: its JSD vectors are filled in SQL row-arrival order, not by topic id
 * (FLOW:1422-1431: similarityVectors[cnt++]), so they are ill-defined -- ours are indexed by topic; its read loop never stores the last
 * entity it reads (FLOW:1418-1433); its pair order is that of a HashMap's key set.
 * Work proceeds in stripes of stripe_rows rows (0: 4096), each with a candidate buffer of candidate_capacity entries (0: 2^22); a stripe
 * that overflows it is redone with a buffer of the size it asked for (stats.regrown counts those).
 * i, j, sim NULL with cap = 0: *count only.  More than cap pairs: MVHDP_ERR_INVALID_ARG, *count set, i / j / sim untouched.  threshold must
 * be finite and >= 0 (else MVHDP_ERR_INVALID_ARG).  The handle supplies device, stream and mvhdp_last_error; no model state is read. */
typedef enum { MVHDP_SIM_COS_FOLDED = 0,  /* 1 - |1 - dot/(|a||b|)|   FLOW:1483, NormalizedDotProductMetric.distance */
               MVHDP_SIM_COS        = 1,  /* dot/(|a||b|)             FLOW:1144, Utils.cosineSimilarity (MatrixOps) */
               MVHDP_SIM_JSD        = 2   /* Maths.jensenShannonDivergence, log base 2   FLOW:1461 */ } mvhdp_sim_metric;
typedef struct { int32_t metric; int32_t n, dim; const double* x /*[n][dim] host*/; double min_weight; double threshold;
                 int32_t stripe_rows /*0: auto*/; int64_t candidate_capacity /*0: auto*/; } mvhdp_sim_args;
typedef struct { int64_t pairs_screened /* matrix cells the first stage computes: 128 x 128 per launched tile (JSD: 16 x 16) */,
                 candidates, emitted; int32_t stripes, regrown; double margin; } mvhdp_sim_stats;
int mvhdp_similar_pairs(mvhdp_handle h, const mvhdp_sim_args* a, int64_t cap, int32_t* i, int32_t* j, double* sim,
                        int64_t* count, mvhdp_sim_stats* stats /* or NULL */);
/* Pure host function, no device: margin, stripes and pairs_screened of a cosine call of that shape (the other fields 0).
 * MVHDP_ERR_INVALID_ARG for n < 0, dim < 1, stripe_rows < 0 or a NULL out; MVHDP_ERR_UNSUPPORTED for dim > 65536. */
int mvhdp_sim_probe(int32_t n, int32_t dim, int32_t stripe_rows, mvhdp_sim_stats* out);

/* findTopicPhrases PTM:1921-1976, which saveTopicsandExperiment calls at PTM:1555 for the 20 most frequent phrases of every topic
 * (PTM:1557-1586) and topicPhraseXMLReport PTM:1978-2070 for the phrase weights and candidate titles: the same-topic word runs of the
 * view-0 tokens, counted per topic.  Only view 0 is read (tokens, z, doc_off as the handle holds them; counts are not), and an entity
 * without view 0 is an empty span.  Per entity, from EMPTY, for every position with (feature, topic): topic == prevtopic starts the phrase
 * [prevfeature, feature] or appends feature to the open one; otherwise an open phrase is counted under prevtopic and the state goes back
 * to EMPTY -- the token that broke the phrase is swallowed, it is not remembered as the start of anything (PTM:1958-1966); otherwise
 * (topic, feature) is remembered (PTM:1968-1969).  Nothing is flushed at the end of the entity: a phrase still open there is dropped.
 * So A A B B B C counts (A: w0 w1) and (B: w3 w4), and A A B B C only the first.  The flow's sequences are plain FeatureSequences: the
 * FeatureSequenceWithBigrams clause of PTM:1951 has no counterpart.  A phrase is its topic and its word-id sequence (the reference's key
 * is the words joined by a blank).
 * Per topic the phrases come by count descending; equal counts by word-id sequence in ascending lexicographic order, a proper prefix
 * first.  THIS tie order is ours: the reference's is the iteration order of a trove hash map seen through RankedFeatureVector.  The list
 * is cut at max_per_topic.  topic_off[k] .. topic_off[k + 1] index counts and word_off; word_off[p] .. word_off[p + 1] index words.
 * distinct[k] = phrases[k].keys().length before the cut; occurrences[k] = the sum of all counts of topic k before the cut (countssum,
 * PTM:2037: the weight of a phrase is count / countssum).  The output is a function of tokens and z alone: two calls give the same bytes.
 * On the device: a walk over the entities (a wave each) that emits one record per occurrence with a 64-bit hash of (topic, length, word
 * ids); a count by key in an open-addressing table sized so that it cannot fill -- the hash places and never decides: two occurrences
 * are one phrase only if topic, length and every word id are equal, compared on the corpus; per topic the phrases that reach the count at
 * the cut.  Only those cross to the host, which settles the order inside equal counts.  stats.hash_collisions counts the comparisons
 * where the used hash bits were equal and the phrases were not (it may differ between two calls; nothing else does).
 * Capacity as mvhdp_doc_topics_top: word_off, words and counts NULL with both caps 0 returns *n_phrases and *n_words (and topic_off /
 * distinct / occurrences / stats, unless NULL); more phrases than cap_phrases or more words than cap_words: MVHDP_ERR_INVALID_ARG, the two
 * sizes set, every array untouched.  word_off holds cap_phrases + 1 entries.
 * MVHDP_ERR_STATE, every output untouched: no view-0 corpus; a view-0 z that is -1 (no assignments yet) or >= K, a view-0 token outside
 * [0, V_0) (the reference throws at alphabet.lookupObject; as mvhdp_diagnostics). */
typedef struct { int32_t max_per_topic;  /* < 0: every phrase (what merging shards needs); the save path uses 20 (PTM:1569) */
                 int32_t hash_bits;      /* 0: 64.  1..63: only that many low bits of the hash are used -- for tests: forces collisions */
               } mvhdp_phrase_args;
typedef struct { int64_t runs /* maximal same-topic runs */, occurrences, distinct, kept, hash_collisions; } mvhdp_phrase_stats;
int mvhdp_topic_phrases(mvhdp_handle h, const mvhdp_phrase_args* a, int64_t cap_phrases, int64_t cap_words,
                        int64_t* topic_off /*[K+1]*/, int64_t* word_off /*[kept+1]*/, int32_t* words, int32_t* counts /*[kept]*/,
                        int64_t* distinct /*[K]*/, int64_t* occurrences /*[K]*/,
                        int64_t* n_phrases, int64_t* n_words, mvhdp_phrase_stats* stats /* or NULL */);

/* Held-out evaluation: the left-to-right document likelihood (Wallach, Murray, Salakhutdinov, Mimno 2009) as MALLET's
 * MarginalProbEstimator.evaluateLeftToRight / leftToRight runs it (mallet-2.0.8 class file), with the arguments getMALLETProbEstimator
 * passes (PTM:3470-3478) -- what replaces getMALLETProbEstimator().evaluateLeftToRight(testing, particles, resample, null).  Defined by its
 * mathematics and this library's random streams; where it departs from MALLET's bytes is said below.
 * The model is view m (0: the only view the reference evaluates) as the handle holds it, frozen for the call: n_wk[m], n_k[m], beta[m],
 * alpha[m][0..K), gamma[m], alphaSum[m].  alphaSum' = gamma[m] * alphaSum[m]; alpha_k = alpha[m][k], NOT multiplied by gamma (the reference
 * passes alpha[0] unscaled beside gamma[0] * alphaSum[0], PTM:3476, and so do we); args.alpha ([K]) with args.alpha_sum replaces both for a
 * caller who wants them consistent.  betaSum = beta[m] * V_m, as MALLET's constructor computes it.  Inactive topics take part with whatever
 * alpha they hold.  A vectors mix (mvhdp_set_vectors_mix) is ignored: the estimator knows nothing of it.  The held-out documents come with
 * the call; the handle's corpus and assignments are neither needed nor touched.
 * Arithmetic, all fp64, every operation rounded on its own (no fused multiply-add), chosen so that a visit has no divide:
 *   rinv[k] = 1.0 / (n_k[k] + betaSum), once per call;  phi_w[k] = (n_wk[w][k] + beta) * rinv[k];  wt[k] = (alpha_k + n_dk[k]) * phi_w[k].
 * Document d (global index doc_base + d), particle r in 0 .. particles - 1: n_dk = 0, tokensSoFar = 0; for limit = 0 .. L - 1:
 *   1. if resample: for every position < limit whose token is in vocabulary (< V_m): take z[position] out of n_dk, form wt for that token,
 *      draw a topic, put it back;
 *   2. the token at limit, out of vocabulary: nothing (no probability, no tokensSoFar increment, no draw); else
 *      p_r[limit] = total / (alphaSum' + tokensSoFar), then tokensSoFar++, z[limit] drawn from wt and added to n_dk.
 * S[n] = sum over r ascending of p_r[n] (0 for an out-of-vocabulary position); the document's log-likelihood is the sum over n with
 * S[n] > 0.0 (the guard of evaluateLeftToRight) of (log S[n] - log particles); the total adds the documents in ascending order.
 * Summation order (part of the contract; tests/native/ltr_ref.c restates this paragraph).  Let T be the smallest of 1, 2, 4, 8, 16, 32 with
 * 64 T >= K.  Lane l (0..63) owns the topics l T + j, j = 0 .. T - 1 (those >= K have weight 0 and are never drawn).  Its prefix sums are
 * pre(l, 0) = wt[l T], pre(l, j) = pre(l, j - 1) + wt[l T + j]; its lane sum is s_l = pre(l, T - 1).  The 64 lane sums are scanned as
 * mvhdp_wave.h's wave_incl_scan_d_dpp does: four steps s = 1, 2, 4, 8 in which every lane with (l mod 16) >= s adds the value lane l - s held
 * before the step; then lanes 16..31 add the value of lane 15 and lanes 48..63 that of lane 47; then lanes 32..63 add the value of lane 31.
 * total = the scanned value of lane 63; excl(l) = the scanned value of lane l - 1, 0.0 for lane 0; the running sum at topic l T + j is
 * excl(l) + pre(l, j).  A draw: u = bits_to_unit(x0, x1) of Philox4x32-10 with key = seed (low word, high word) and counter
 * (low 32 bits of doc_base + d,  r + (high 32 bits of doc_base + d) * 2^20,  limit,  position), position = limit for the draw at the limit;
 * the topic is the first one in ascending order with wt > 0.0 whose running sum exceeds u * total; if there is none, the last topic with
 * wt > 0.0 (topic 0 if every weight is 0).  The per-document sum: with the terms t_n = log S[n] - log particles of the positions that pass
 * the guard, lane l adds t_l, t_(l + 64), .. in ascending order from 0.0, and the 64 lane values are combined by a butterfly (each lane adds
 * the value of lane l xor 32, then 16, 8, 4, 2, 1); the device's log is within an ulp of a correctly rounded one, not equal to it.
 * Departures from MALLET: its typeTopicCounts argument is decoded as packed (count << topicBits) | topic words, which the reference's dense
 * int[V][K] rows are not -- we read n_wk[w][k]; MALLET walks SparseLDA buckets (smoothing, document, word), which gives the same
 * distribution with a different map from u to topic -- we do not reproduce that map; its Randoms is unseeded -- ours is the counter above;
 * it divides per topic -- we multiply by rinv (an ulp of difference per weight at most).
 * doc_off[0] = 0 and doc_off[num_docs] tokens; a token >= V_m is out of vocabulary.  doc_ll [num_docs], position_sum [N] (S[n]),
 * doc_tokens [num_docs] (in-vocabulary tokens) and stats may each be NULL.  stats.visits counts the weight vectors formed, over all
 * particles: sum over documents and limits of (in-vocabulary positions < limit, if resample) + (1 if the limit's token is in vocabulary).
 * Pending work on the handle's stream lands first.  The counts are taken AS THE HANDLE HOLDS THEM: unlike mvhdp_diagnostics this call
 * does not refuse counts that have gone stale (assignments replaced since the last count) or that lack the pending deltas of a
 * MVHDP_SWEEP_NO_APPLY sweep -- it evaluates the table as it stands, i.e. the model before that sweep; call mvhdp_apply_delta (or
 * mvhdp_build_counts) first to evaluate the newer one.  MVHDP_ERR_STATE: no counts yet (mvhdp_build_counts, mvhdp_set_counts, or a sweep) or
 * no hyper-parameters; MVHDP_ERR_UNSUPPORTED: K > 2048 (checked with the arguments; mvhdp_create admits no such K); MVHDP_ERR_INVALID_ARG: m out of range, particles < 1 (or > 2^20), a negative token, a doc_off that does not start
 * at 0 or decreases, a negative doc_base; -1 for a NULL handle.  Every output is untouched on error.  The counts, the assignments, the tuning
 * and what mvhdp_counts_written / mvhdp_trees_current would report are what they were; two calls with the same arguments return the same bytes.
 * Cost: sum over documents of particles * L (L + 1) / 2 visits with resample, particles * L without; each visit gathers one count row. */
typedef struct { int32_t m, particles, resample; uint64_t seed; int64_t doc_base;
                 const double* alpha /*[K] or NULL*/; double alpha_sum; } mvhdp_heldout_args;
typedef struct { double log_likelihood; int64_t tokens /* in vocabulary */, oov, visits; } mvhdp_heldout_stats;
int mvhdp_heldout_left_to_right(mvhdp_handle h, const mvhdp_heldout_args* a, int64_t num_docs,
        const int64_t* doc_off /*[D+1]*/, const int32_t* tokens /*[N]*/,
        double* doc_ll /*[D] or NULL*/, double* position_sum /*[N] or NULL: S[n], 0 for OOV*/,
        int64_t* doc_tokens /*[D] or NULL*/, mvhdp_heldout_stats* stats);

/* Fold-in: the topic proportions of a batch of UNSEEN documents over the M views, on the trained handle, in one call: tokens to theta.  The
 * rows feed mvhdp_nearest_entities (args.queries) and mvhdp_predict_items (args.theta) as they are.  The reference's route
 * (inferTopicDistributionsOnNewDocs INF:114-330: a second model, inference trees, frozen sweeps) stays available through a second handle
 * (mvhdp_set_counts, mvhdp_build_inference_trees, mvhdp_init_assignments_from_trees, MVHDP_SWEEP_FROZEN, mvhdp_doc_topic_proportions);
 * THIS definition is ours: the reference sampler's conditional written densely over all K topics, a chain of our own;
 * tests/native/foldin_ref.c restates this paragraph sequentially and the device equals it bit for bit.
 * Model: n_wk[m], n_k[m], beta[m], betaSum[m], gamma[m], alpha[m][0..K), alphaSum[m] of every view and inActiveTopicIndex, frozen for the
 *   call and taken AS THE HANDLE HOLDS THEM -- the state rule of mvhdp_heldout_left_to_right: MVHDP_ERR_STATE without counts or
 *   hyper-parameters; stale counts and the pending deltas of a MVHDP_SWEEP_NO_APPLY sweep are neither refused nor applied.  A vectors mix
 *   (mvhdp_set_vectors_mix) is ignored (the inferencer's worker runs with lambda = 0, INF:251-252).  The documents come with the call; the
 *   handle's corpus and assignments are neither needed nor touched.
 * Document d (global id doc_base + d): its view-m span is tokens[m][doc_off[m][d] .. doc_off[m][d + 1]); doc_off[m] == NULL: no document
 *   has view m (every span empty).  len_m = the span's length, out-of-vocabulary tokens included (the length mvhdp_doc_topic_proportions
 *   uses).  A token >= V_m is out of vocabulary: never visited, holds no topic (z = -1 in the output), in no count.  Every other token
 *   starts unassigned.
 * Weights, all fp64, every operation rounded on its own (no fused multiply-add):
 *   a_m[k] = gamma[m] * alpha[m][k];  Lp_m = (double)len_m + gamma[m] * alphaSum[m];  rinv_m[k] = 1.0 / ((double)n_k[m][k] + betaSum[m]),
 *   once per call;  phi_{m,w}[k] = ((double)n_wk[m][w][k] + beta[m]) * rinv_m[k], and exactly 0.0 for a topic in inActiveTopicIndex
 *   (PTM:2670-2671), which is therefore never drawn.
 * Coupling: P = args.coupling, [M][M] row-major on the host, every entry finite and >= 0 (else MVHDP_ERR_INVALID_ARG).  With NULL:
 *   P[m][m] = 1, P[m][i] = p_a[m][i] / (p_a[m][i] + p_b[m][i]) of the handle's hyper-parameters (the mean of the reference's per-entity
 *   Beta draw, WRK:331-333, unrounded), and 0 where p_a[m][i] == 0.
 * One iteration (it = 1 .. iterations): views in ascending m, within a view the positions in ascending order (WRK:393,425).  At the start
 *   of view m's pass, from the CURRENT counts of the other views (WRK:395-410, the same operation order), for every topic k:
 *     s = 0.0;  for i ascending, i != m, len_i != 0:  s = s + P[m][i] * ((double)n_dk[i][k] + a_i[k]) / Lp_i   (product, then quotient);
 *     o_m[k] = s * Lp_m;  base_m[k] = a_m[k] + o_m[k].
 *   A view with len_m == 0 has no pass.  A visit of an in-vocabulary token w at position pos: if the token has a topic, take it out of
 *   n_dk[m];  wt[k] = (P[m][m] * (double)n_dk[m][k] + base_m[k]) * phi_{m,w}[k];  draw a topic, give it to the token and add it to
 *   n_dk[m].  A visit has no divide.
 * Draw: lane ownership (T, lane l owns the topics l T + j), the in-lane prefix sums, the wave scan, total, and "the first topic in
 *   ascending order with wt > 0.0 whose running sum exceeds u * total, else the last topic with wt > 0.0" are exactly the summation-order
 *   paragraph of mvhdp_heldout_left_to_right above.  total == 0.0 or not finite: the token is left as it was before the visit (an
 *   unassigned one stays unassigned and uncounted).  u = bits_to_unit(x0, x1) of Philox4x32-10 with key = seed (low word, high word) and
 *   counter (low 32 bits of doc_base + d,  high 32 bits of doc_base + d,  it + m * 2^16,  pos): a document's draws depend on nothing but
 *   its global id, the seed and its own tokens.
 * Samples: S = args.samples >= 1, args.thin >= 1; the recorded states are those after the iterations iterations - (S - 1 - s) * thin,
 *   s = 0 .. S - 1; each of them must be >= 1 and iterations >= 1 (else MVHDP_ERR_INVALID_ARG).  counts_sum[d][m][k] = the integer sum of
 *   n_dk[m][k] over the recorded states.  S = 1: the final state, as the reference reports; S > 1: the average of MALLET's
 *   getSampledDistribution, which a six-token side view needs.
 * theta[d][k]: the expression of mvhdp_doc_topic_proportions, the same operations in the same order, with n_dk[m][k] replaced by
 *   (double)counts_sum[d][m][k] / (double)S (the count itself for S = 1) and len_m as above.  Every view takes part as present: an empty
 *   span scores with zeros, as mvhdp_set_view_presence = 1 does; nothing carries over between documents.  view_weights as in that entry:
 *   finite, none negative, their sum > 0 (else MVHDP_ERR_INVALID_ARG); it may be NULL when theta is NULL.
 * z[m][n]: the final state of every position (-1: out of vocabulary or unassigned); z, or any z[m], may be NULL.  stats: tokens (in
 *   vocabulary) and oov over all views; visits = weight vectors formed = tokens * iterations; kernel_ms = the kernel's time on the stream.
 * mvhdp_foldin_args, in this order: int32 iterations, samples, thin; uint64 seed; int64 doc_base; the two host pointers (48 bytes with
 *   the padding behind thin); mvhdp_foldin_stats: three int64 and a double (32 bytes).  tests/test_foldin_kats.py pins both.
 * Limits: K <= MVHDP_MAX_TOPICS, M <= 8, iterations <= 65535 (the counter's 16 bits), a span of at most 2^31 - 1 tokens, otherwise any
 *   length.  MVHDP_ERR_INVALID_ARG: a NULL args, doc_off or tokens array, a negative num_docs, token or doc_base, a doc_off[m] that does
 *   not start at 0 or decreases, the cases named above; -1 for a NULL handle.  num_docs == 0: MVHDP_OK.  Every output is untouched on error.
 * Guarantees: two calls with the same arguments return the same bytes (kernel_ms aside); a document's result does not depend on which
 *   other documents share the call; the counts, the assignments, the tuning and what mvhdp_counts_written / mvhdp_trees_current would
 *   report are what they were.  Pending work on the handle's stream lands first.
 * Departures from the frozen-sweep inferencer: the reference adds the other views' mass only for the topics in the document's non-zero
 *   list, which never grows during a visit, and reaches gamma * alpha * p_wt through a stored tree and a three-way branch -- we form the
 *   same sum densely over every topic; it draws p per entity from Beta(0.2, 1), rounded to three decimals, from a stream that cannot be
 *   seeded (INF:221-224, WRK:331-336) -- we take a fixed matrix; it zeroes the coupling of a view whose beta == 0.0001 (WRK:335-336) -- we
 *   do not, the caller passes a zero; its initial topics come from trees of p_wt alone (INF:169-199) -- ours come from the first
 *   iteration's visits of unassigned tokens; its out-of-vocabulary tokens keep topic 0 and are counted in it by printDocumentTopics --
 *   ours hold none.
 * Cost: tokens * iterations visits, each gathering one count row; device scratch is bounded per chunk of documents (mvhdp_foldin.hip). */
typedef struct { int32_t iterations, samples, thin; uint64_t seed; int64_t doc_base;
                 const double* coupling /*[M][M] host, or NULL*/;
                 const double* view_weights /*[M], or NULL without theta*/; } mvhdp_foldin_args;
typedef struct { int64_t tokens /* in vocabulary */, oov, visits; double kernel_ms; } mvhdp_foldin_stats;
int mvhdp_fold_in(mvhdp_handle h, const mvhdp_foldin_args* a, int64_t num_docs,
        const int64_t* const* doc_off /*[M] -> [num_docs+1]; an entry may be NULL: no document has that view*/,
        const int32_t* const* tokens /*[M] -> [N_m]*/,
        double* theta /*[num_docs][K] or NULL*/, int32_t* const* z /*[M] -> [N_m]; entries or the array itself may be NULL*/,
        int32_t* counts_sum /*[num_docs][M][K] or NULL*/, mvhdp_foldin_stats* stats /* or NULL */);

/* Cross-view prediction: the types of view m ranked per entity by the model's own expectation, score(d, w) = sum_k theta_d[k] * phi[w][k].
 * The reference has no counterpart (its flow ends at the similarity SQL): THIS definition is ours; tests/native/xview_ref.c restates it.
 * theta_d[k]: the bits of mvhdp_doc_topic_proportions(h, view_weights, d, d + 1), its missing-view carry-over included.  A caller who
 *   predicts view m from the other views passes view_weights[m] = 0.  The weights must be finite, none negative, their sum > 0 (else
 *   MVHDP_ERR_INVALID_ARG).  args.theta, a host array [d1 - d0][K], replaces the proportions (view_weights may then be NULL); every entry
 *   must be finite and >= 0 (else MVHDP_ERR_INVALID_ARG).
 * phi[w][k] = ((double)n_wk[m][w][k] + beta[m]) / ((double)n_k[m][k] + betaSum[m]): one correctly rounded fp64 division; exactly 0.0 for a
 *   topic in inActiveTopicIndex (PTM:2670-2671).  A vectors mix (mvhdp_set_vectors_mix) is NOT applied.
 * score(d, w): s = +0.0; for k = 0 .. K - 1 ascending: s = fma(theta_d[k], phi[w][k], s) -- a fused fp64 multiply-add per topic, one chain,
 *   no partial sums, no reassociation.
 * Order of the view's types for an entity: score descending, equal scores by ascending type id.  (The comparison is that of the 64-bit
 *   pattern made monotone -- sign bit set for a non-negative score, every bit flipped for a negative one -- which is the numeric order of
 *   any two scores; with the arguments admitted above every score is finite and >= +0.0.)
 * Excluded set of d (only with exclude_present != 0): the types < V_m that occur in d's view-m span of the handle's corpus.  They are never
 *   listed and never counted in a rank.
 * mvhdp_predict_items: per entity of [d0, d1) the first min(n, V_m - |excluded|) types in that order with their scores; counts[d - d0] says
 *   how many; unused slots hold item -1 and score 0.0.  n >= 1; n > V_m is allowed.  On the device the list is placed by counting, for each
 *   listed type, the listed types in front of it: n is meant to be small (the cost per entity grows with n^2 / 64).
 * mvhdp_score_items: for pair i, score[i] = score(entity[i], item[i]), the same bits, and rank[i] = the number of types w' != item[i] of
 *   view m that are not excluded for entity[i] and precede item[i] in the order (0-based).  The queried item is scored and ranked even
 *   when it is itself excluded.  Pairs may come in any order and repeat; only entities that have pairs are computed.  Log-score, recall@N
 *   and reciprocal rank are the host's to derive.
 * Preconditions: as mvhdp_doc_topic_proportions (every view's corpus, the hyper-parameters), and counts that are current: no counts yet,
 *   stale counts, or the pending deltas of a MVHDP_SWEEP_NO_APPLY sweep return MVHDP_ERR_STATE, as mvhdp_diagnostics does.
 * MVHDP_ERR_INVALID_ARG, every output untouched: m out of range, a bad entity range, a NULL output, n < 1, a pair whose entity is outside
 *   [d0, d1) or whose item is outside [0, V_m), bad weights or theta.  d0 == d1 or n_pairs == 0: MVHDP_OK, nothing written.
 * No model state changes.  Integers and exact fp64 values decide every comparison: two calls give the same bits.
 * On the device: phi formed once per call as fp64 [V_m][K] (in stripes of types beyond 256 MiB); a tiled fp64 kernel computes a block of
 * scores [entities][V_m] (at most 256 MiB at a time; the D x V_m matrix never exists whole); one wave per entity selects behind it. */
typedef struct { int32_t m; int32_t exclude_present; const double* view_weights /*[M] or NULL with theta*/;
                 const double* theta /*[d1-d0][K] host, or NULL*/; } mvhdp_predict_args;
int mvhdp_predict_items(mvhdp_handle h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, int32_t n,
                        int32_t* items /*[d1-d0][n]*/, double* scores /*[d1-d0][n]*/, int32_t* counts /*[d1-d0]*/);
int mvhdp_score_items(mvhdp_handle h, const mvhdp_predict_args* a, int64_t d0, int64_t d1, int64_t n_pairs,
                      const int64_t* entity /*[n_pairs], in [d0,d1), any order, repeats allowed*/, const int32_t* item /*[n_pairs], in [0,V_m)*/,
                      double* score /*[n_pairs]*/, int32_t* rank /*[n_pairs]*/);

/* Entities for an item: the candidate entities [c0, c1) of this handle ranked per QUERY by the same expectation, taken from the item's side:
 * score(d, j) = sum_k theta_d[k] * psi_j[k], psi_j a weighted set of phi rows of view m (a tag, a cited paper, a few query words) or a row
 * of the caller's.  The reference has no counterpart: THIS definition is ours; tests/native/xview_entities_ref.c restates it.
 * theta_d[k]: the bits of mvhdp_doc_topic_proportions(h, view_weights, d, d + 1), its missing-view carry-over included; formed on the device
 *   in blocks and never shipped to the host.  view_weights: finite, none negative, their sum > 0; a caller who predicts view m from the
 *   other views passes view_weights[m] = 0.
 * phi[w][k]: exactly that of mvhdp_predict_items -- one correctly rounded division, exactly 0.0 for a topic in inActiveTopicIndex.  A
 *   vectors mix is NOT applied.
 * Query row psi_j[k], item form (psi == NULL): query j is the list q_items[q_off[j] .. q_off[j + 1]) with weights c_i = q_weights[i] (1.0
 *   with q_weights == NULL):  p = +0.0; for i ascending: p = fma(c_i, phi[w_i][k], p).  One item of weight 1.0 gives the bits of phi[w][k].
 *   Every item must lie in [0, V_m) (unlike a corpus token, an item >= V_m is an error); every weight finite, >= 0 and <= 2^53; a query
 *   holds at most 2^20 items, so psi stays finite.  Repeated items are allowed and each occurrence adds.  An empty query is a row of zeros.
 *   Host form (psi != NULL): the caller's rows [nq][K], every entry finite and >= 0 -- a topic mixture, or phi rows of another model;
 *   q_off, q_items, q_weights and exclude_present are then ignored.
 * score(d, j): s = +0.0; for k = 0 .. K - 1 ascending: s = fma(theta_d[k], psi_j[k], s) -- one fused fp64 chain, no partial sums, no
 *   reassociation.  For a one-item weight-1 query it is mvhdp_score_items' score(d, w) in every bit (the product commutes inside the fma).
 * Order of the candidates for a query: score descending, equal scores by ascending entity id; compared by the monotone 64-bit pattern, as for
 *   mvhdp_predict_items.  With the arguments admitted every score is finite and >= +0.0.
 * Excluded for query j (item form with exclude_present != 0 only): an entity whose view-m span in the handle's corpus holds at least one
 *   item of query j.  Excluded entities are never listed and never counted in a rank.
 * mvhdp_predict_entities: per query the first min(n, candidates not excluded) entities in that order -- ids of this handle and their
 *   scores; counts[j] says how many; unused slots hold id -1 and score 0.0.  1 <= n <= 1024; n > c1 - c0 is allowed.
 * mvhdp_rank_entities: for pair i, score[i] = score(entity[i], query[i]), the same bits, and rank[i] = the number of candidates
 *   d != entity[i] of [c0, c1) that are not excluded for that query and precede entity[i] in the order (0-based).  The queried entity is
 *   scored and ranked even when it is itself excluded.  It must lie in [c0, c1), the query index in [0, nq).  Pairs may repeat and come in
 *   any order; only queries that have pairs are computed.  Cost: n_pairs x (c1 - c0) comparisons, behind the scores of every candidate
 *   for every query that has a pair.
 * Preconditions: as mvhdp_predict_items (every view's corpus, the hyper-parameters, counts that are current), else MVHDP_ERR_STATE.
 * MVHDP_ERR_INVALID_ARG, every output untouched: a NULL args or output; a bad view or candidate range; nq < 0; n outside 1..1024; a q_off
 *   that does not start at 0 or decreases; a bad item, weight or psi entry; bad view weights; a negative block_entities or block_queries;
 *   a bad pair.  -1 for a NULL handle.  MVHDP_ERR_UNSUPPORTED: 2^31 candidates or more.  nq == 0 or n_pairs == 0: MVHDP_OK, only stats
 *   written.  c0 == c1: every count 0.  Pending work on the handle's stream lands first.
 * On the device: queries in blocks of block_queries (0: 4096), candidates in blocks of block_entities (0: 8192, a query's row of keys then
 *   fits the selection's 64 KiB of LDS; a longer row is selected from memory), the block of scores [queries][entities] within 256 MiB (the
 *   knobs are cut to that).  The tiled fp64 kernel of mvhdp_predict_items computes the block with the roles swapped; one wave per query
 *   merges the block's first n with the n carried from the blocks before.  The knobs change no result.  No floating-point atomics: two calls
 *   with the same arguments return the same bytes (kernel_ms aside).  Nothing of the handle moves: the counts, the assignments, the
 *   tuning and what mvhdp_counts_written / mvhdp_trees_current would report are what they were.
 * stats (or NULL): cells = scores computed; excluded = (entity, query) cells marked; blocks = blocks of scores; kernel_ms = the stream's
 *   time from the first kernel to the last.
 * mvhdp_entities_args, in this order: int32 m, exclude_present; the view_weights pointer; int64 c0, c1, nq; the four host pointers q_off,
 *   q_items, q_weights, psi; int64 block_entities, block_queries (88 bytes).  mvhdp_entities_stats: two int64, an int32, a double
 *   (32 bytes with the padding behind blocks).  tests/test_xview_entities_kats.py pins both. */
typedef struct { int32_t m; int32_t exclude_present; const double* view_weights /*[M]*/; int64_t c0, c1;      /* candidate entities [c0, c1) */
                 int64_t nq; const int64_t* q_off /*[nq+1]*/; const int32_t* q_items; const double* q_weights /* or NULL: every weight 1.0 */;
                 const double* psi /*[nq][K] host, or NULL*/; int64_t block_entities /*0: auto*/, block_queries /*0: auto*/; } mvhdp_entities_args;
typedef struct { int64_t cells /* scores computed */, excluded /* (entity, query) cells marked */; int32_t blocks; double kernel_ms; } mvhdp_entities_stats;
int mvhdp_predict_entities(mvhdp_handle h, const mvhdp_entities_args* a, int32_t n, int64_t* ids /*[nq][n]*/, double* scores /*[nq][n]*/,
                           int32_t* counts /*[nq]*/, mvhdp_entities_stats* stats /* or NULL */);
int mvhdp_rank_entities(mvhdp_handle h, const mvhdp_entities_args* a, int64_t n_pairs, const int64_t* query /*[n_pairs]*/, const int64_t* entity /*[n_pairs]*/,
                        double* score /*[n_pairs]*/, int64_t* rank /*[n_pairs]*/);

/* Nearest entities: for each of nq query rows the n entities of [c0, c1) of this handle with the largest cosine similarity.  The reference
 * only compares groups (its Java double loop, FLOW:1320-1532, cannot do more): THIS definition is ours; tests/nearest_numpy.py restates it.
 * It is pinned to the arithmetic of mvhdp_similar_pairs, so every value can be checked against that entry point bit for bit.
 * Candidate rows: theta of the entities [c0, c1), the bits of mvhdp_doc_topic_proportions(h, view_weights, ..), its missing-view carry-over
 *   included.  They are computed on the device and stay there: nothing of size [entities][K] crosses to the host.
 * Query rows: args.queries, a host array [nq][K] (for example the proportions of folded-in documents from an inference handle); or, with
 *   queries == NULL, the entities [q0, q1) of this same handle (nq = q1 - q0; args.nq is ignored).  In that form exclude_self != 0 removes
 *   an entity from its own list; with host rows exclude_self is ignored.
 * min_weight as in mvhdp_similar_pairs: an entry <= min_weight of a query or candidate row counts as 0; -inf: none.  NaN: MVHDP_ERR_INVALID_ARG.
 * sim(q, c): the bits of MVHDP_SIM_COS in mvhdp_similar_pairs -- dot = the unfused fp64 chain s = s + q_k * c_k over ascending k from +0.0,
 *   |row| = sqrt of the same chain of squares, sim = dot / (|q| * |c|).
 * Order per query: sim descending, equal sims by ascending entity id.  (The comparison is that of the 64-bit pattern made monotone, as for
 *   mvhdp_predict_items; the chain never yields -0.0 from rows without negative zeros.)
 * Never listed: a candidate whose norm is 0, Inf or NaN; a pair whose sim is NaN (only where fp64 over- or underflows).  A query whose norm
 *   is 0, Inf or NaN gets counts[q] = 0.
 * counts[q] = min(n, candidates that may be listed); ids[q][0 .. counts[q]) are entity ids of this handle, sims[q][.] their values; the
 *   unused tail holds id -1 and sim 0.0.  n >= 1; n > c1 - c0 is allowed.  n is meant to be small: per query the list is placed by counting,
 *   for each listed entity, the listed ones in front of it (n^2 / 64), and the device keeps 32 n bytes per query of a block.
 * Two stages, as in mvhdp_similar_pairs; the screen never decides.
 * (a) Screen, on the matrix cores: rows normalised in fp64, stored as fp32, a block of queries against a stripe of candidates in
 *   rectangular 128 x 128 tiles with v_mfma_f32_32x32x2_f32 (one fp32 fma chain over every k).  Per query row let tau be the n-th largest
 *   screen value over its screened candidates that may be listed (the query itself left out when exclude_self applies).  Candidates of the
 *   exact stage are the cells with screen >= tau - margin, margin = (K + 4) * 2^-23, the margin of mvhdp_similar_pairs: it is twice the
 *   bound b on |screen - exact|; n cells have screen >= tau, so their exact values are >= tau - b and so is the n-th largest exact value;
 *   every member of the true first n, ties at the n-th place included, therefore has screen >= tau - 2 b.  Fewer than n screened cells:
 *   all of them.  With more than one stripe, a stripe is cut with the n-th largest screen value over the stripes SO FAR, this one included:
 *   a value <= tau, hence a superset of the cells above (and the same set when one stripe holds every candidate).
 *   A row with a non-zero |entry| outside [2^-500, 2^500] is not screened: such a candidate is a candidate of every query, such a query
 *   takes every candidate.  stats.exact_only_rows counts those rows, query rows and candidate rows each.
 * (b) Exact: every candidate recomputed by the fp64 chain; a wave per query selects the first n by (sim descending, id ascending).
 * Work proceeds in blocks of block_queries queries (0: 8192; at most 2^26 / stripe) times stripes of stripe_candidates candidates
 * (0 or more than 8192: 8192), each block with a candidate buffer of candidate_capacity entries (0: 2^22); a block that overflows it is
 * redone with a buffer of the size it asked for (stats.regrown counts those).  The knobs change no result.  Device memory: 12 K bytes per
 * query and per candidate row (the fp64 rows and their fp32 image, for the whole call), a block of screen values of at most 256 MiB, and
 * 24 bytes per candidate of a block.
 * stats (or NULL): cells_screened = matrix cells of the first stage (128 x 128 per launched tile); candidates = entries of the exact
 * stage over all blocks; exact_only_rows; blocks; regrown; margin.
 * Preconditions as mvhdp_doc_topic_proportions: every view's corpus and the hyper-parameters (else MVHDP_ERR_STATE).
 * MVHDP_ERR_INVALID_ARG, every output untouched: a NULL args, view_weights, ids, sims or counts; n < 1; a candidate range outside
 * [0, D] or c0 > c1; with queries == NULL a query range outside [0, D] or q0 > q1; with host rows nq < 0; a NaN min_weight; a negative
 * block_queries, stripe_candidates or candidate_capacity.  MVHDP_ERR_UNSUPPORTED: K > 65536; 2^31 - 128 query or candidate rows or more.
 * nq == 0: MVHDP_OK, only stats written.  c0 == c1: every count 0.  No model state changes; two calls give the same bits. */
typedef struct { const double* view_weights /*[M]*/; int64_t c0, c1; const double* queries /*[nq][K] host, or NULL: entities [q0, q1)*/;
                 int64_t nq, q0, q1; int32_t exclude_self, n; double min_weight;
                 int32_t block_queries /*0: auto*/, stripe_candidates /*0: auto*/; int64_t candidate_capacity /*0: auto*/; } mvhdp_nearest_args;
typedef struct { int64_t cells_screened, candidates, exact_only_rows; int32_t blocks, regrown; double margin; } mvhdp_nearest_stats;
int mvhdp_nearest_entities(mvhdp_handle h, const mvhdp_nearest_args* a, int64_t* ids /*[nq][n]*/, double* sims /*[nq][n]*/,
                           int32_t* counts /*[nq]*/, mvhdp_nearest_stats* stats /* or NULL */);
/* Pure host function, no device: margin, blocks and cells_screened of a call with nq query rows, nc candidates and K topics (the other
 * fields 0).  MVHDP_ERR_INVALID_ARG for nq < 0, nc < 0, K < 1, a negative block_queries or stripe_candidates, or a NULL out;
 * MVHDP_ERR_UNSUPPORTED for K > 65536. */
int mvhdp_nearest_probe(int64_t nq, int64_t nc, int32_t K, int32_t block_queries, int32_t stripe_candidates, mvhdp_nearest_stats* out);
/* Top entities per topic: for every topic k the n entities d of [d0, d1) with the largest theta_d[k], theta the bits of
 * mvhdp_doc_topic_proportions(h, view_weights, ..).  Ours as well (tests/nearest_numpy.py).  Order: weight descending, equal weights by
 * ascending entity id.  Only weights > threshold are kept, strictly; -inf keeps every entity; NaN: MVHDP_ERR_INVALID_ARG.  1 <= n <= 1024.
 * counts[k] = min(n, entities kept); ids[k][0 .. counts[k]) and weights[k][.]; the unused tail holds id -1 and weight 0.0.  Inactive
 * topics are listed like any other (their proportions are what mvhdp_doc_topic_proportions gives).
 * On the device theta is produced in chunks of chunk_entities entities (0: as many as fit 256 MiB, also the most); a thread per topic and
 * slice of slice_entities entities (0: 2048), lanes over topics so that the row-major reads coalesce, keeps the first n of its slice; one
 * wave per topic merges the slices.  The knobs change no result.  No floating-point atomics: two calls give the same bits.
 * MVHDP_ERR_INVALID_ARG, every output untouched: a NULL buffer, a bad range, n outside 1..1024, a NaN threshold, a negative chunk_entities
 * or slice_entities.  MVHDP_ERR_UNSUPPORTED: 2^31 entities or more.  Preconditions as mvhdp_doc_topic_proportions.  d0 == d1: every count 0. */
int mvhdp_topic_top_entities(mvhdp_handle h, const double* view_weights /*[M]*/, int64_t d0, int64_t d1, int32_t n, double threshold,
                             int64_t chunk_entities /*0: auto*/, int64_t slice_entities /*0: auto*/,
                             int64_t* ids /*[K][n]*/, double* weights /*[K][n]*/, int32_t* counts /*[K]*/);

/* The topic map: Gram sums and co-occurrence counts of every pair of topics over a tall matrix X with K columns -- which topics are
 * near-duplicates by their word distributions (the question behind mergeSimilarTopics PTM:677-843 and CalcTopicSimilarities
 * FLOW:1084-1196), which topics occur together in the same entities (the topic graph a front end draws).  The reference has no
 * counterpart with a fixed order: THIS definition is ours; tests/native/gram_ref.c restates it.
 * Rows X_r[k], r in [r0, r1), by args.source:
 *   MVHDP_GRAM_ENTITIES: the bits of mvhdp_doc_topic_proportions(h, view_weights, r, r + 1), its missing-view carry-over included;
 *     0 <= r0 <= r1 <= D; preconditions as that entry (every view's corpus, the hyper-parameters, else MVHDP_ERR_STATE); view_weights
 *     finite, none negative, their sum > 0.  m is ignored.
 *   MVHDP_GRAM_WORDS: phi[r][k] of view m exactly as mvhdp_predict_items defines it -- one correctly rounded division, exactly 0.0 for a
 *     topic in inActiveTopicIndex; a vectors mix is NOT applied; 0 <= r0 <= r1 <= V_m.  The counts must be current and no NO_APPLY delta
 *     pending, else MVHDP_ERR_STATE, as in that entry.
 *   MVHDP_GRAM_HOST: the caller's rows x [r1 - r0][K], every entry finite and >= 0; 0 <= r0 <= r1.  The handle supplies the device and
 *     the stream only (and K).
 * Transform: y_r[k] = X_r[k] (MVHDP_GRAM_IDENTITY) or sqrt(X_r[k]), correctly rounded (MVHDP_GRAM_SQRT).  With SQRT over WORDS gram[k][l]
 *   is the Bhattacharyya coefficient of two topics' word distributions (Hellinger = sqrt(1 - BC) on the host); with IDENTITY
 *   gram[k][l] / sqrt(gram[k][k] * gram[l][l]) is their cosine; with IDENTITY over ENTITIES gram, sums and stats.rows give the Pearson
 *   correlation of two topics across entities.
 * Order.  All arithmetic is fp64 and every operation is rounded on its own except the fma named here.  Block b holds the rows
 *   [r0 + b * B, min(r0 + (b + 1) * B, r1)), B = MVHDP_GRAM_BLOCK_ROWS.
 *   Block partial: p = +0.0; for r ascending in the block: p = fma(y_r[k], y_r[l], p)  -- one fused chain, no partial sums inside a block.
 *   gram[k][l]: g = +0.0; for b ascending: g = g + P_b[k][l].
 *   sums[k]: the same two levels with plain adds: q = +0.0; q = q + y_r[k] inside a block; then the blocks ascending.
 *   Why there are blocks: one chain over 10^6 rows is serial.  A partial per 1024 rows is the unit of parallelism, and its size is part of
 *   the definition.  The result is symmetric in every bit, because the product commutes inside the fma.
 *   blocks_per_pass: how many block partials live on the device at once; 0: as many as fit 256 MiB.  Either way a pass is cut so that its
 *   rows fit 1 GiB.  It changes no result.
 * Integers, both taken on X, before the transform, and the comparison is strict:
 *   n_above[k] = #{r : X_r[k] > threshold};  co_above[k][l] = #{r : X_r[k] > threshold and X_r[l] > threshold}, so co_above[k][k] =
 *   n_above[k].  A NaN threshold: MVHDP_ERR_INVALID_ARG; -inf counts every row, +inf none.  Either output may be NULL; with both NULL
 *   that work is skipped.
 * MVHDP_ERR_INVALID_ARG, every output untouched: a NULL args, gram or sums; a bad source, transform, m (WORDS) or range; a negative
 *   blocks_per_pass; bad view weights (ENTITIES); a NULL x or a bad x entry (HOST).  -1 for a NULL handle.  MVHDP_ERR_UNSUPPORTED: more
 *   than 2^40 rows.  r0 == r1: MVHDP_OK, all outputs zero, blocks == 0.  Pending work on the handle's stream lands first.  Nothing of
 *   the handle moves: the counts, the assignments, the tuning and what mvhdp_counts_written / mvhdp_trees_current would report are what
 *   they were.  No floating-point atomics: two calls with the same arguments give the same bytes (kernel_ms aside).
 * On the device: per pass theta (or phi, or the caller's rows) is formed for blocks_per_pass blocks and stays there.  A workgroup owns one
 *   block of rows and one tile of 64 x 128 cells (k, l), each thread 4 x 8 fp64 accumulators fed by vector fp64 fma from slabs of 16
 *   rows in LDS -- the tile kernel of mvhdp_predict_items without its transposition, X being row-major over the topics; only tiles on and
 *   above the diagonal run.  A small kernel then adds the pass's partials into gram and sums in ascending block order, one thread per
 *   cell.  Counts: a ballot over 64 rows gives per topic a 64-bit mask of the rows above the threshold, a block is 16 such words per
 *   topic, and co_above[k][l] grows by popcount(mask_k & mask_l) through integer atomics (integer adds commute, so they stay exact).
 * stats (or NULL): rows = r1 - r0; blocks = blocks of rows; passes; kernel_ms = the stream's time from the first kernel to the last.
 * mvhdp_topic_gram_args, in this order: int32 source, m, transform, blocks_per_pass; the pointers view_weights and x; int64 r0, r1; double
 *   threshold (56 bytes).  mvhdp_topic_gram_stats: an int64, two int32, a double (24 bytes).  tests/test_gram_kats.py pins both. */
#define MVHDP_GRAM_BLOCK_ROWS 1024
typedef enum { MVHDP_GRAM_ENTITIES = 0, MVHDP_GRAM_WORDS = 1, MVHDP_GRAM_HOST = 2 } mvhdp_gram_source;
typedef enum { MVHDP_GRAM_IDENTITY = 0, MVHDP_GRAM_SQRT = 1 } mvhdp_gram_transform;
typedef struct { int32_t source, m, transform, blocks_per_pass /*0: auto*/;
                 const double* view_weights /*[M], ENTITIES only*/; const double* x /*[r1-r0][K] host, HOST only*/;
                 int64_t r0, r1; double threshold; } mvhdp_topic_gram_args;
typedef struct { int64_t rows; int32_t blocks, passes; double kernel_ms; } mvhdp_topic_gram_stats;
int mvhdp_topic_gram(mvhdp_handle h, const mvhdp_topic_gram_args* a, double* gram /*[K][K]*/, double* sums /*[K]*/,
                     int64_t* n_above /*[K] or NULL*/, int64_t* co_above /*[K][K] or NULL*/, mvhdp_topic_gram_stats* stats /* or NULL */);

/* ---- topic diagnostics: the step after training (FastQMVWVTopicModelDiagnostics, DIAG = MVTopicModel/FastQMVWVTopicModelDiagnostics.java;
 * SciTopicFlow builds it with N = 20 right after the save, whose saveExperiment / saveTopicsandExperiment call
 * calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230 from PTM:1370 / PTM:1507 and getSortedWords PTM:1792-1811 per view).
 * Preconditions as mvhdp_model_log_likelihood: counts current, no pending NO_APPLY delta (else MVHDP_ERR_STATE).  Integer outputs
 * are exact; fp64 outputs follow the reference's formulas; every sum is taken in a fixed order (no floating-point atomics), so two
 * calls give the same bits.  Outputs are written only when the call succeeds.  DIAG reads view 0 only (alpha[0], gamma[0], beta[0],
 * tokensPerTopic[0], the view-0 tokens), even for an M-view model; so does mvhdp_diagnostics. ---- */
#define MVHDP_DIAG_MAX_TOP_WORDS 64
#define MVHDP_DIAG_PROPORTIONS   7       /* DEFAULT_DOC_PROPORTIONS {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5}, DIAG:27 */
/* score rows, the order of DIAG:104-116 */
#define MVHDP_DIAG_TOKENS             0  /* tokensPerTopic[0][k]                                DIAG:242-250 */
#define MVHDP_DIAG_DOCUMENT_ENTROPY   1  /* -sumCountTimesLogCount[k] / T + log T               DIAG:252-260 */
#define MVHDP_DIAG_WORD_LENGTH        2  /* mean length of the top N words, / N always          DIAG:462-483 (NaN without word_length) */
#define MVHDP_DIAG_COHERENCE          3  /* log((D(i,j) + beta0) / (D(j,j) + beta0)) over j < i  DIAG:544-571 */
#define MVHDP_DIAG_NORM_DISCR_WEIGHT  4  /* discrWeight / |log10 alpha0[k] - log10 avg alpha0|  DIAG:313-338 (avg over K+1 entries, zeros not counted) */
#define MVHDP_DIAG_DISCR_WEIGHT       5  /* calcDiscrWeightWithinTopics(.., true)[0][k]          DIAG:297-311, PTM:2233-2270 */
#define MVHDP_DIAG_UNIFORM_DIST       6  /*                                                     DIAG:262-295 */
#define MVHDP_DIAG_CORPUS_DIST        7  /*                                                     DIAG:368-404 */
#define MVHDP_DIAG_EFF_NUM_WORDS      8  /*                                                     DIAG:340-363 */
#define MVHDP_DIAG_TOKEN_DOC_DIFF     9  /*                                                     DIAG:406-457 */
#define MVHDP_DIAG_RANK_1_DOCS       10  /* rank-1 documents / non-zero documents               DIAG:573-581 */
#define MVHDP_DIAG_ALLOCATION_RATIO  11  /* documents at 50 % / documents at 2 %                DIAG:583-598 */
#define MVHDP_DIAG_ALLOCATION_COUNT  12  /* documents at 30 % / non-zero documents              DIAG:600-613 */
#define MVHDP_DIAG_ROWS              13
typedef struct {
    int32_t num_top_words;               /* N, 1..MVHDP_DIAG_MAX_TOP_WORDS (DIAG uses 20, saveTopicsandExperiment 49) */
    const int32_t* word_length;          /* [V_0] String.length() of every view-0 type (UTF-16 code units), or NULL: the word-length row is NaN */
} mvhdp_diag_args;
typedef struct {                         /* caller-owned; every pointer but `scores` may be NULL (not wanted) */
    double*  scores;                     /* [MVHDP_DIAG_ROWS][K] TopicScores.scores; a row left alone by DIAG stays 0 (discrWeight rows of alpha0[k] == 0) */
    double*  word_scores;                /* [MVHDP_DIAG_ROWS][K][N] TopicScores.topicWordScores (0 for the rows that define none) */
    int32_t* codoc;                      /* [K][N][N] topicCodocumentMatrices DIAG:122,209-221 */
    int32_t* top_types;                  /* [K][N] view-0 top words as mvhdp_top_words(h, 0, N, ..) */
    int32_t* top_counts;                 /* [K][N] */
    int32_t* nonzero;                    /* [K] */
    int32_t* num_rank1_docs;             /* [K] DIAG:228-230 */
    int32_t* num_nonzero_docs;           /* [K] DIAG:189 */
    int32_t* num_docs_at_proportions;    /* [K][MVHDP_DIAG_PROPORTIONS] DIAG:199-204 */
    double*  sum_count_log_count;        /* [K] DIAG:196 */
    int32_t* word_type_counts;           /* [V_0] DIAG:171 */
    int64_t* num_tokens;                 /* [1] DIAG:170 */
    double*  discr_weight_per_view;      /* [M] as mvhdp_discr_weights */
} mvhdp_diag_out;
/* getSortedWords(m) PTM:1792-1811 cut at n (1..64): per topic the types with n_wk > 0 by count descending, equal counts by DESCENDING
 * type id (IDSorter.compareTo); types/counts [K][n], unfilled slots -1 / 0; nonzero[k] = sortedWords.size(). */
int mvhdp_top_words(mvhdp_handle h, int32_t m, int32_t n, int32_t* types /*[K][n]*/, int32_t* counts /*[K][n]*/, int32_t* nonzero /*[K]*/);
/* calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230: per_view[v] = skewSum / nonZeroSkewCnt with BOTH accumulators carried across
 * views and nonZeroSkewCnt starting at 1 (the reference's running mean over views 0..v) -- discrWeightPerModality, the view weight
 * factor of printDocumentTopics / the inferencer (PTM:2890-2898, INF:402-411; mvhdp_doc_topic_proportions).  type_weight: [V_m]
 * typeDiscrWeight[m][w] = sum_k n_wk^2 / (sum_k n_wk)^2 (0 for an empty row), or NULL. */
int mvhdp_discr_weights(mvhdp_handle h, double* per_view /*[M]*/, int32_t m, double* type_weight /*[V_m] or NULL*/);
/* The diagnostics of DIAG:53-117: getSortedWords of view 0 cut at N, collectDocumentStatistics DIAG:120-236 over the view-0 tokens,
 * the thirteen score rows.  Quirks kept: the top-N position of a topic with fewer than N words holds type 0 (DIAG:132,146-150), so it
 * counts as present in a document whenever type 0 is one of the topic's real top words and occurs with it there; the rank-1 topic is
 * the lowest index among equal counts; proportions (gamma0 alpha0[k] + c) / (gamma0 alphaSum0 + len) unfused; empty or inactive topics
 * give the NaN / Inf Java gives.  wordTypeCounts are the view-0 row sums of n_wk (equal to the token counts when the counts are current;
 * checked against tokensPerTopic[0]).  A view-0 token that is unassigned (-1) or out of the vocabulary is refused (DIAG:171-173 throws):
 * MVHDP_ERR_STATE, outputs untouched. */
int mvhdp_diagnostics(mvhdp_handle h, const mvhdp_diag_args* args, mvhdp_diag_out* out);

/* ---- topic words per cohort: what a topic looks like inside a set of entities -- its words in the papers of one year, its tags and cited
 * papers (views 1 and 2) at one venue, its vocabulary in one author's work.  The counterpart in token units of the "Trends" of
 * CalcEntityTopicDistributionsAndTrends (FLOW:807-1083, mvhdp_entity_topic_distributions); the definition is ours.
 * A cohort is a list of entity ids, in the CSR form of mvhdp_entity_topic_distributions: cohort g lists members[member_off[g] ..
 *   member_off[g + 1]).  An entity may be listed in several cohorts and more than once in one cohort; every listing counts.
 * What is read: tokens, z and doc_off of view m as the handle holds them -- the rule of mvhdp_topic_phrases: whatever the last sweep left on
 *   the device, live or deferred.  An entity without view m is an empty span.  Only listed entities are read.
 * A token is counted when 0 <= type < V_m and 0 <= z < K.  A token with z == -1 or type >= V_m is skipped; stats.skipped counts the skipped
 *   tokens once per listing.  A z outside [-1, K) or a negative type in a listed entity: MVHDP_ERR_STATE.
 * Per cohort g and topic k:
 *   c_g[w][k]     = the counted tokens of type w and topic k, summed over the listings of g;
 *   tokens[g][k]  = sum_w c_g[w][k] (the trend in token units);
 *   docs[g][k]    = the listings of g whose entity holds at least one counted token of topic k in view m;
 *   nonzero[g][k] = the types with c_g[w][k] >= 1.
 * The list of (g, k): the types with c_g[w][k] >= min_count in the chosen order, cut at n; unfilled slots hold -1 / 0, as in
 *   mvhdp_top_words.
 *   MVHDP_COHORT_BY_COUNT: count descending, equal counts by descending type id (IDSorter.compareTo, the order of mvhdp_top_words).
 *   MVHDP_COHORT_BY_SHARE: by the exact rational c_g[w][k] / n_wk[m][w][k] descending -- the part of the word's topic-k tokens that lies in
 *     the cohort -- compared by 64-bit cross products, never by a floating-point quotient; equal shares by count descending, then by
 *     descending type id.  BY_COUNT returns mostly a topic's head words in every cohort; the share order shows a cohort's own vocabulary,
 *     and min_count keeps singletons out of it.
 * Preconditions: a corpus of view m (else MVHDP_ERR_STATE); BY_COUNT needs nothing else, no counts and no hyper-parameters.  BY_SHARE also
 *   needs current counts and no pending MVHDP_SWEEP_NO_APPLY delta, the rule of mvhdp_top_words, else MVHDP_ERR_STATE.
 * MVHDP_ERR_INVALID_ARG: a NULL args or member_off; m out of range; n outside 1..MVHDP_DIAG_MAX_TOP_WORDS; min_count < 1; scratch_bytes < 0;
 *   an order that is neither value; one of types / counts NULL and the other not; n_cohorts < 0; member_off[0] != 0 or member_off
 *   decreasing; a member outside [0, D); the listings of one cohort holding more than 2^31 - 1 tokens of view m, counted or not (summed on
 *   the host from the spans' lengths before any device work: a count cell cannot overflow).  -1 for a NULL handle.
 *   MVHDP_ERR_UNSUPPORTED: more than 16384 topics.  n_cohorts == 0 (after these checks): MVHDP_OK.  Every output is untouched on any error.
 * scratch_bytes bounds the device scratch of the count tables, one [K][V_m] int32 table per cohort of a pass; 0: 1 GiB.  A value smaller
 *   than one table means one cohort per pass, never an error.  It changes no result.
 * Guarantees: integers only, so two calls with the same arguments return the same bytes (kernel_ms aside); a cohort's result does not
 *   depend on which other cohorts share the call; nothing of the handle moves: the counts, the assignments, the tuning and what
 *   mvhdp_counts_written / mvhdp_trees_current would report are what they were.  Pending work on the handle's stream lands first.  With
 *   types, counts and nonzero all NULL only the trends (tokens, docs) are computed and no count table is needed.
 * Cost: one pass over the listed tokens (8 bytes read per token, an int32 atomic into the table, one atomic each into tokens and docs per
 *   listing and topic seen), plus per cohort one clear and one scan of a K x V_m int32 table: 8 K V_m bytes per cohort.
 * On the device: one wave per listing, lanes over the span's tokens; the table is topic-major, so the selection -- one block per cohort and
 *   topic, the sorted top-n list of mvhdp_top_words per wave -- reads a topic's column contiguously, and BY_SHARE reads n_wk only for
 *   the types that reach min_count.  Outputs are staged and copied out once, after the whole call has succeeded.
 * stats (or NULL): listings = member_off[n_cohorts]; tokens = the counted tokens over all listings; skipped; passes; cohorts_per_pass;
 *   kernel_ms = the stream's time from the first kernel to the last.
 * mvhdp_cohort_args, in this order: int32 m, n, order, min_count; int64 scratch_bytes (24 bytes).  mvhdp_cohort_stats: int64 listings,
 *   tokens, skipped; int32 passes, cohorts_per_pass; double kernel_ms (40 bytes).  tests/test_cohort_kats.py pins both. */
typedef enum { MVHDP_COHORT_BY_COUNT = 0, MVHDP_COHORT_BY_SHARE = 1 } mvhdp_cohort_order;
typedef struct { int32_t m, n, order, min_count; int64_t scratch_bytes /*0: auto*/; } mvhdp_cohort_args;
typedef struct { int64_t listings, tokens, skipped; int32_t passes, cohorts_per_pass; double kernel_ms; } mvhdp_cohort_stats;
int mvhdp_cohort_top_words(mvhdp_handle h, const mvhdp_cohort_args* a, int64_t n_cohorts, const int64_t* member_off /*[n_cohorts+1]*/,
                           const int64_t* members, int32_t* types /*[G][K][n] or NULL*/, int32_t* counts /*[G][K][n] or NULL*/,
                           int32_t* nonzero /*[G][K] or NULL*/, int64_t* tokens /*[G][K] or NULL*/, int64_t* docs /*[G][K] or NULL*/,
                           mvhdp_cohort_stats* stats /* or NULL */);

/* ---- word-set co-occurrence: in how many windows of a corpus the words of a set occur, alone and in pairs -- the integer counts behind the
 * UCI, NPMI and UMass coherence measures (Newman 2010, Lau 2014, Roeder 2015) over documents or over a Boolean sliding window, on the
 * training corpus or on a held-out or reference corpus, for any view, and independent of the assignments.  The coherence inside
 * mvhdp_diagnostics (codoc, DIAG:209-221) counts a top word only where the token is assigned to the topic, in view 0, per document; this call
 * gives a merged topic and its parents, the two sides of a split or two models the same yardstick.  The reference has no counterpart; the
 * definition is ours.  The formulas stay on the host: the device returns integers.
 * Word sets: n_sets rows of n slots, n in 1..MVHDP_DIAG_MAX_TOP_WORDS -- exactly the types[K][n] that mvhdp_top_words and
 *   mvhdp_diagnostics.top_types return, -1 slots included.  A slot holds a type of view m or -1; a -1 may sit anywhere in a row, and its row and
 *   column of co stay 0.  A word may sit in any number of sets, and in several slots of one set: then every such slot counts.
 * Corpus: the caller's or the handle's.  The caller's is doc_off / tokens / num_docs, host arrays in the CSR form of mvhdp_fold_in for the
 *   single view m -- a held-out or reference corpus.  With doc_off == NULL the corpus is tokens and doc_off of view m as the handle holds
 *   them; num_docs and tokens are then ignored.  z is never read; counts and hyper-parameters are never needed.  Only the entities [d0, d1)
 *   of whichever corpus are read; d1 == -1: to its end.
 * Tokens: a token with type >= V_m is out of the vocabulary: it occupies its position and matches no slot.  A negative type is an error:
 *   MVHDP_ERR_INVALID_ARG in the caller's corpus, MVHDP_ERR_STATE in the handle's.
 * Windows, for an entity whose span has L tokens: L == 0 gives no window.  window == 0 gives one window, the whole span (document
 *   co-occurrence).  window == W >= 1 is the Boolean sliding window: its starts are i = 0 .. max(L - W, 0), and window i covers the positions
 *   [i, min(i + W, L)).  So a span no longer than W is one window and a longer one has L - W + 1.  *windows = the windows over the range.
 * Counts: slot (s, i) is present in a window when some position of the window holds its word.  co[s][i][j] = the windows in which the slots i
 *   and j of set s are both present; co[s][i][i] = the windows in which slot i is present.  The matrix is symmetric, every cell is int64,
 *   and a cell never exceeds *windows: nothing can overflow (the device adds into 64-bit cells).
 * stats (or NULL): entities = the non-empty spans read; tokens = the positions read; hits = the positions whose type sits in at least one
 *   set; oov = the positions with type >= V_m; distinct_words = the distinct types over all sets; memberships = the filled slots;
 *   kernel_ms = the stream's time from the first kernel to the last.
 * MVHDP_ERR_INVALID_ARG, in this order: a NULL a, co or windows, n_sets < 0, sets NULL with n_sets > 0; m out of range, n outside 1..64,
 *   window < 0; a slot < -1 or >= V_m; with a caller's corpus num_docs < 0, NULL tokens with tokens to read, doc_off not starting at 0 or
 *   decreasing, a negative token; d0 < 0, d1 < -1, d0 > d1 (after -1 is resolved), d1 beyond the corpus.  MVHDP_ERR_UNSUPPORTED:
 *   n_sets * n * n > 2^26 cells.  MVHDP_ERR_STATE: the handle's corpus asked for and mvhdp_set_corpus(m) not called.  -1 for a NULL handle.
 *   n_sets == 0 or an empty range, after the checks: MVHDP_OK, with *windows still counted and co untouched (it has no cells) or all zeros.
 *   Every output is untouched on any error.
 * Guarantees: integers only, so two calls with the same arguments return the same bytes (kernel_ms aside); a set's result does not
 *   depend on which other sets share the call; results are additive over disjoint entity ranges, because a window never crosses an
 *   entity; nothing of the handle moves: the assignments, the counts, alpha, the tuning and what mvhdp_counts_written /
 *   mvhdp_trees_current report are what they were.  Pending work on the handle's stream lands first.  Outputs are staged and copied out
 *   once, after the whole call has succeeded.
 * On the device: the sets become an inverted index (first[V_m + 1], packed (set, slot) memberships); one wave per entity, longest first,
 *   lanes over positions.  An entity goes in chunks of 64 window starts with a 64-bit coverage word per present slot: an occurrence at p
 *   covers the starts [p - W + 1, p], one run of bits, and a pair gets one add of popcount(cov_i & cov_j) per chunk; no window is visited
 *   on its own.  A caller's corpus goes up in chunks of whole documents with bounded scratch.
 * mvhdp_cooc_args, in this order: int32 m, n, window (4 bytes of padding); int64 d0, d1 (32 bytes).  mvhdp_cooc_stats: int64 entities,
 *   tokens, hits, oov; int32 distinct_words, memberships; double kernel_ms (48 bytes).  tests/test_cooc_kats.py pins both. */
typedef struct { int32_t m, n, window; int64_t d0, d1 /*-1: to the end*/; } mvhdp_cooc_args;
typedef struct { int64_t entities, tokens, hits, oov; int32_t distinct_words, memberships; double kernel_ms; } mvhdp_cooc_stats;
int mvhdp_word_cooccurrence(mvhdp_handle h, const mvhdp_cooc_args* a, int64_t n_sets, const int32_t* sets /*[n_sets][n], -1 = empty slot*/,
                            int64_t num_docs, const int64_t* doc_off /*[num_docs+1], or NULL: the handle's corpus of view m*/,
                            const int32_t* tokens, int64_t* co /*[n_sets][n][n]*/, int64_t* windows /*[1]*/, mvhdp_cooc_stats* stats /* or NULL */);

/* ---- topic surgery: merge, drop and reorder topics on the trained handle.  mvhdp_topic_gram finds near-duplicate topics, mvhdp_diagnostics
 * junk topics, n_k the topics that have died out; this call acts on them.  It is what the reference's mergeSimilarTopics (PTM:677-843, left
 * commented out there) does with its merge map and delete list -- every z rewritten (PTM:832-834), then a recount -- applied to the
 * assignments, the counts, alpha and the inactive set together, on the device.  The definition is ours.
 * One hop: z' = map[z] for z >= 0; -1 stays -1.  map[k] in [0, K) is the topic that takes topic k's tokens, MVHDP_UNASSIGNED_TOPIC drops
 *   them (they become unassigned, and the next sampling sweep assigns them anew).  The map is NOT chased: map = [1, 2, 2] sends topic 0's
 *   tokens to 1 and topic 1's to 2.  Any map is legal, permutations with cycles included.  The sources of t are {k : map[k] == t}.
 * Counts: n_wk'[w][t] = the sum of n_wk[w][k] over the sources of t, n_k' likewise: after the call the counts are exactly the recount of
 *   z' (mvhdp_build_counts would change nothing).
 * alpha: for every view, alpha'[m][t] = the fp64 sum of alpha[m][k] over the sources of t in ascending k; a single source moves its bits, so
 *   a permutation permutes alpha exactly.  A topic without a source gets +0.0.  alpha[m][K], alpha_sum and every other field of mvhdp_hyper
 *   stay as they are: the mass of dropped topics is NOT redistributed (the host does that through mvhdp_set_hyper if it wants to).
 * inactive: a topic with sources is inactive iff all its sources were.  A topic without a source keeps its state -- an active one stays
 *   "active" with alpha 0 and is never sampled again, as PTM:751 leaves it -- unless MVHDP_REMAP_RETIRE is set: then it joins the inactive
 *   set, and a later birth can take its index (a truncated HDP otherwise never gets a vacated index back).  first_inactive is recomputed
 *   and MVHDP_BUF_BIRTH_KEYS is reset to MVHDP_ACT_KEY_NONE.
 * The handle afterwards: as after mvhdp_set_assignments of every view and mvhdp_build_counts -- the counts current, the trees outdated, the
 *   slot counts, the 16-bit and 12-bit images and the row classes rewritten by the next sweep's own preparation.  Every kind of sweep goes
 *   on from there and equals, integer for integer, a fresh handle loaded with z', alpha', inactive' (tests/test_gpu_remap.py).
 * Refusals, checked whole before anything changes (z, counts, alpha and inactive stay byte for byte): MVHDP_ERR_INVALID_ARG for a NULL a
 *   or map, an entry below -1 or >= K, an unknown flag; MVHDP_ERR_STATE before mvhdp_set_corpus of every view or mvhdp_set_hyper, with
 *   counts that are not current or a MVHDP_SWEEP_NO_APPLY sweep's deltas pending (the rule of mvhdp_top_words), inside an
 *   mvhdp_apply_delta_begin bracket; MVHDP_ERR_UNSUPPORTED while a vectors mix is set (its [V_0][K] columns belong to topics) or embeddings
 *   with topic rows are initialised (mvhdp_emb_release first).  -1 for a NULL handle.
 * stats (or NULL): moved[m] = the view-m tokens whose z changed to another topic, dropped[m] = those that became unassigned; vacated = the
 *   topics without a source that held tokens or were active before, retired = those of them that are inactive afterwards; kernel_ms = the
 *   stream's time over both passes.
 * On the device: one pass over every view's z (the map in LDS, 16-byte loads, a lane stores only what changed) and one over the sumV + M
 *   rows of MVHDP_BUF_COUNTS, a wave per row, the row held in registers and folded through LDS in place: 4 bytes read per token and per
 *   count cell, written only where something changed.  profiles/remap_topics.md has the figures.
 * Not done: the reference's own discriminative-weight delete rule (PTM:773-809: the host builds the map, mvtopicmodel_amd/surgery.py has
 *   merge, prune and order maps), a JNI class.  Splitting a topic is mvhdp_split_topic below.
 * mvhdp_remap_args: a pointer and a uint32 (16 bytes).  mvhdp_remap_stats: int64 moved[8], dropped[8]; int32 vacated, retired; double
 *   kernel_ms (144 bytes).  tests/test_remap_kats.py pins both. */
#define MVHDP_REMAP_RETIRE 0x1u   /* vacated topics join the inactive set (ours); without it they stay active with alpha 0, as PTM:751 leaves them */
typedef struct {
    const int32_t* map;     /* [K]: map[k] in [0, K) = the topic that takes topic k's tokens; MVHDP_UNASSIGNED_TOPIC = they become unassigned */
    uint32_t flags;
} mvhdp_remap_args;
typedef struct {
    int64_t moved[MVHDP_MAX_MODALITIES];    /* tokens whose z changed to another topic */
    int64_t dropped[MVHDP_MAX_MODALITIES];  /* tokens that became unassigned */
    int32_t vacated, retired;               /* topics no topic maps onto that held tokens or were active before; of those, inactive afterwards */
    double kernel_ms;
} mvhdp_remap_stats;
int mvhdp_remap_topics(mvhdp_handle h, const mvhdp_remap_args* a, mvhdp_remap_stats* stats /* or NULL */);

/* ---- topic surgery, the opposite move: cut one topic in two on the trained handle, with a Gibbs sampler restricted to the tokens of that
 * topic and to two outcomes.  The reference has no counterpart (its unfinished mergeSimilarTopics only merges): THIS definition is ours;
 * tests/native/split_ref.c restates this paragraph sequentially and the device equals it integer for integer and bit for bit.  For a
 * truncated HDP a split is also the deliberate form of a birth: the target is a free index, usually one of the inactive set.
 * The split set: every position n of every view m with z[m][n] == source.  Every other position and every other topic's counts stay byte
 *   for byte as they were.  During the call a token of the set carries a side, a (it stays in source) or b (it goes to target).
 * The target: a topic index != source that holds no token in any view (n_k[m][target] == 0) and whose alpha[m][target] is exactly 0.0 in
 *   every view, else MVHDP_ERR_INVALID_ARG.  target == -1: the library picks the lowest index of the inactive set that meets these
 *   conditions; MVHDP_ERR_INVALID_ARG ("no free topic") if there is none.
 * Constants of the call, per view, fp64, every operation rounded on its own (no fused multiply-add):
 *   ah_m = 0.5 * alpha[m][source];  A_m = gamma[m] * ah_m, the same for both sides;  Lp_m = (double)len_m + gamma[m] * alphaSum[m] per
 *   entity, len_m the entity's WHOLE view-m span, as in mvhdp_fold_in;  P = args.coupling: exactly the fold-in's matrix, its default for
 *   NULL and its validation.
 * Iteration 0, the initial sides: a token of type w with type_hint[m][w] == 0 or 1 takes that side; every other token (hint -1, a NULL
 *   row, a NULL array) takes b iff u >= 0.5, else a.  u = bits_to_unit(x0, x1) of Philox4x32-10 with key = seed (low word, high word) and
 *   counter (low 32 bits of g,  high 32 bits of g,  it + m * 2^16,  pos), g = doc_id_base + d, it = 0, pos = the position inside the
 *   entity's view-m span: the fold-in's counter.  A hint value outside {-1, 0, 1}: MVHDP_ERR_INVALID_ARG.
 * Iteration it = 1 .. iterations: the word counts are FROZEN for the whole iteration (the library's deferred discipline):
 *   c_w[m][w][x] and c[m][x], x in {a, b}, are the counts of the sides as the previous iteration left them; per view and side two
 *   reciprocals per iteration, r0 = 1.0 / ((double)c[m][x] + betaSum[m]) and r1 = 1.0 / ((double)(c[m][x] - 1) + betaSum[m]).  Entities
 *   are independent of each other within an iteration.  Inside an entity the views go in ascending m and within a view the positions of the
 *   split set in ascending order; the entity's own side counts e[m][x] are LIVE.  At the start of view m's pass, for x in {a, b}, in the
 *   fold-in's operation order:
 *     s = 0.0;  for i ascending, i != m, len_i != 0:  s = s + P[m][i] * ((double)e[i][x] + A_i) / Lp_i   (product, then quotient);
 *     base[x] = A_m + s * Lp_m.
 *   A view in which the entity has no token of the set has no pass.  A visit of a token of type w currently on side y: take it out of
 *   e[m][y];  for each x with own = (x == y):  phi[x] = ((double)(c_w[m][w][x] - own) + beta[m]) * (own ? r1 : r0)[x];
 *   wt[x] = (P[m][m] * (double)e[m][x] + base[x]) * phi[x];  total = wt[a] + wt[b];  the token goes to a iff u * total < wt[a], else to
 *   b, u as above with this it;  total == 0.0 or not finite: the token keeps y;  add it to e[m] of its new side.  A visit has no divide.
 *   flips[it - 1] = the tokens whose side changed in iteration it.
 * Afterwards: z holds source or target for the set; the counts are exactly the recount of the new z (mvhdp_build_counts would change
 *   nothing); alpha'[m][source] = alpha'[m][target] = ah_m (0.5 a + 0.5 a == a bitwise unless ah_m is subnormal) -- with
 *   MVHDP_SPLIT_KEEP_ALPHA the source keeps its alpha and the target gets ah_m, and alpha_sum is the host's business, as after
 *   mvhdp_remap_topics.  alpha[m][K], alpha_sum and every other field of mvhdp_hyper are untouched.  The target leaves the inactive set
 *   (stats.activated), first_inactive is recomputed and MVHDP_BUF_BIRTH_KEYS is reset to MVHDP_ACT_KEY_NONE.  The handle is in the state
 *   mvhdp_remap_topics leaves: the counts current, the trees outdated, the slot counts, the 16-bit and 12-bit images and the row classes
 *   rewritten by the next sweep's own preparation; every kind of sweep goes on from there and equals, integer for integer, a fresh
 *   handle loaded with z', alpha', inactive' (tests/test_gpu_split.py).
 * Refusals, checked whole before anything changes (z, counts, alpha and inactive stay byte for byte): those of mvhdp_remap_topics --
 *   MVHDP_ERR_STATE before mvhdp_set_corpus of every view or mvhdp_set_hyper, with counts that are not current or a MVHDP_SWEEP_NO_APPLY
 *   sweep's deltas pending, inside an mvhdp_apply_delta_begin bracket; MVHDP_ERR_UNSUPPORTED while a vectors mix is set, embeddings with
 *   topic rows are initialised, or K > 2048 -- and MVHDP_ERR_INVALID_ARG for a NULL a, source or target out of range (target below -1 or
 *   >= K), source == target, a source in the inactive set, an unknown flag, iterations outside 0 .. 65535 (the counter's 16 bits), a bad
 *   coupling or hint, the target's conditions above.  -1 for a NULL handle.  A source without tokens is MVHDP_OK with zeros: the target
 *   is still activated and alpha still halved.
 * stats (or NULL): split[m] = the view-m tokens of the set, moved[m] = of those, in the target at the end; flips_last = flips of the last
 *   iteration (0 with iterations == 0); target = the index used, activated = 1 if it left the inactive set; kernel_ms = the stream's time
 *   over the kernels of the call.
 * Guarantees: two calls with the same arguments on the same state give the same bytes (kernel_ms aside); an entity's draws depend on
 *   nothing but its global id, the seed, its own tokens and the frozen counts, so a later group form (the counts of the sides summed
 *   over the shards between iterations) can equal one handle.
 * On the device (mvhdp_split.hip): one pass over every view's z with 16-byte loads lists the set in entity order (position, type, side
 *   byte) with a CSR by entity; the word counts of the two sides live in a table [sumV + M][2] of int32 filled from the source column;
 *   per iteration one sampling launch (a wave per entity that owns tokens of the set, chunks of 64 records, the chain resolved from LDS)
 *   and one launch of integer atomics on the table; at the end z of the set and the two columns of the count rows are written.
 *   profiles/split_topic.md has the figures.
 * Not done: mvhdp_group_split_topic / NativeGroup.split_topic, a JNI class.
 * mvhdp_split_args, in this order: int32 source, target, iterations; uint32 flags; uint64 seed; two host pointers (40 bytes).
 *   mvhdp_split_stats: int64 split[8], moved[8], flips_last; int32 target, activated; double kernel_ms (152 bytes).
 *   tests/test_split_kats.py pins both. */
#define MVHDP_SPLIT_KEEP_ALPHA 0x1u   /* the source keeps its alpha; the target still gets 0.5 * alpha[m][source] */
typedef struct {
    int32_t source, target;              /* target: a topic index, or -1 = the library picks the lowest free index of the inactive set */
    int32_t iterations;                  /* 0 .. 65535 restricted sweeps after the initial assignment */
    uint32_t flags;
    uint64_t seed;
    const double* coupling;              /* [M][M] host or NULL: exactly mvhdp_fold_in's P and its default */
    const int8_t* const* type_hint;      /* NULL, or [M] -> NULL or [V_m]: -1 none, 0 stays in source, 1 starts in target */
} mvhdp_split_args;
typedef struct {
    int64_t split[MVHDP_MAX_MODALITIES]; /* tokens of view m that carried the source topic */
    int64_t moved[MVHDP_MAX_MODALITIES]; /* of those, in the target at the end */
    int64_t flips_last;                  /* tokens that changed side in the last iteration (0 with iterations == 0) */
    int32_t target, activated;           /* the target used; 1 if it left the inactive set */
    double kernel_ms;
} mvhdp_split_stats;
int mvhdp_split_topic(mvhdp_handle h, const mvhdp_split_args* a, int64_t* flips /*[iterations] or NULL*/, mvhdp_split_stats* stats /* or NULL */);

/* ---- word and topic embeddings: trainTypeVectors (PTM:517-524, 1186-1206, 1495-1498) and SciTopicFlow.runWordEmbeddings (FLOW:115-136).
 * TWE = MVTopicModel/TopicWordEmbeddings.java, TWER = MVTopicModel/TopicWordEmbeddingRunnable.java.  WordEmbeddings is TWE with no
 * topics and no context columns: the same trainer with with_topics = 0 (a WordEmbeddings host makes a K = 1, M = 1 handle over its
 * text).  Rows: the V_0 word rows, then (with topics) the K topic rows; weights and negative weights [R][C] in fp64 on the device.
 * Skip-gram with negative sampling over view 0 plus the terms that tie each token to its topic (TWER:261-291); tokens and z are read
 * straight from the handle.  Every draw comes from Philox4x32-10.  A group of document shards has no form of
 * this: a member trains on its own entities only.  The softmax table p_emb(w|t) stays on the device for the useVectorsLambda mix of
 * the sweep: mvhdp_set_vectors_mix(h, lambda, NULL, NULL) below hands it to the samplers. ---- */
typedef struct {
    int32_t num_columns;                 /* C, 1..256 (PTM:523 vectorSize; FLOW:74 uses 200) */
    int32_t num_context_columns;         /* Cc, 0 <= Cc < C: columns [0, Cc) "context", [Cc, C) "content" (50); ignored without topics (TWE:136) */
    int32_t with_topics;                 /* 1: TopicWordEmbeddings (R = V_0 + K), 0: WordEmbeddings (R = V_0) */
    int32_t window;                      /* windowSize >= 1 (5) */
    int32_t num_samples;                 /* negatives per call, 0..32 (5) */
    int32_t min_doc_length;              /* entities keeping fewer tokens are skipped, >= 1 (10) */
    int64_t sampling_table_size;         /* 1..2^31-1 (10^8) */
    double  sampling_factor;             /* countWords(data, f) (1e-4) */
    double  min_exp, max_exp;            /* sigmoid bounds (-6, 6) */
    int32_t sigmoid_cache_size;          /* 1..4096 (1000) */
    int32_t reserved;                    /* 0 */
} mvhdp_emb_config;
typedef struct {                         /* one mvhdp_emb_train, summed over its epochs */
    int64_t words_so_far;                /* view-0 tokens visited (TWER:243) */
    int64_t words_sampled;               /* tokens kept by the subsampling (TWER:251) */
    int64_t words_considered;            /* kept tokens of the entities not skipped (TWER:263) */
    int64_t docs_skipped;                /* entities keeping fewer than min_doc_length tokens (TWER:257) */
    int64_t calls;                       /* gradientLearn calls (numUpdates TWER:146) */
    int64_t negatives_skipped;           /* negative draws equal to the input row (TWER:119) */
    double  residual;                    /* sum of the residuals (TWER:114,142); getMeanError = residual / calls */
    double  last_epoch_residual;         /* the same over the last epoch */
    int64_t last_epoch_calls;
    double  kernel_ms;
} mvhdp_emb_stats;
#define MVHDP_EMB_SERIAL 0x1u            /* one wave, entities in id order: deterministic, the restatement's order.  Default: Hogwild */
/* new TopicWordEmbeddings(alphabet[0], C, Cc, window, K, ..) TWE:126-163 / new WordEmbeddings WE:119-145: weights = (u - 0.5) / C
 * (or the caller's [R][C]) and negative weights 0; the sigmoid cache TWE:157-162 with cache[size] left 0.0.  Replaces any earlier state. */
int mvhdp_emb_init(mvhdp_handle h, const mvhdp_emb_config* cfg, const double* weights /*[R][C] or NULL*/, uint64_t seed);
/* countWords(data, f) TWE:341-401 over the handle's view-0 tokens: wordCounts and totalWords cumulative over calls (kept quirk),
 * retention[w] = min((sqrt(s) + 1) / s, 1) with s = count / (f total), the sampling table equal index for index to the reference's. */
int mvhdp_emb_count_words(mvhdp_handle h);
/* train(data, threads, num_samples, epochs) TWE:423-483 with TWER:82-293: `epochs` passes over the entities in id order.  Learning rate
 * of entity d in epoch e: max(0.025e-4, 0.025 (1 - (e N_0 + doc_off[d]) / (epochs totalWords))).  seed and round select the streams.
 * MVHDP_ERR_INVALID_ARG, vectors untouched, for a view-0 token outside [0, V_0) or, with topics, a z outside [0, K). */
int mvhdp_emb_train(mvhdp_handle h, int32_t epochs, uint64_t seed, uint32_t round, uint32_t flags, mvhdp_emb_stats* stats /* or NULL */);
/* getWordVectors / getTopicVectors TWE:726-745 (the rows from V_0 on are the topics), writeContext, checkpoints.  Either may be NULL. */
int mvhdp_emb_get_vectors(mvhdp_handle h, double* weights /*[R][C]*/, double* negative_weights /*[R][C]*/);
int mvhdp_emb_set_vectors(mvhdp_handle h, const double* weights /*[R][C]*/, const double* negative_weights /*[R][C]*/);
/* probes of countWords: cumulative counts [V_0], retention [V_0], totalWords; table entries [first, first + n) */
int mvhdp_emb_word_stats(mvhdp_handle h, int64_t* counts /* or NULL */, double* retention /* or NULL */, int64_t* total_words /* or NULL */);
int mvhdp_emb_sampling_table(mvhdp_handle h, int64_t first, int64_t n, int32_t* types /*[n]*/);
/* CalcSoftmaxTopicWordProbabilities PTM:337-367 (with topics): dot over all C columns of word row w and topic row t, exp(dot - max_w dot)
 * kept on the device as [V_0][K]; sum_exp[t] accumulates over calls as PTM:360 does (reset_sums = 1: from 0).  Copies may be NULL. */
int mvhdp_emb_softmax(mvhdp_handle h, int32_t reset_sums, double* exp_dot /*[K][V_0]*/, double* sum_exp /*[K]*/);
/* findClosest(v) TWE:485-540: the n (1..64) word rows and topic rows of highest cosine against query [C] in IDSorter order (cosine
 * descending, ties by descending id); slots beyond V_0 / K hold -1 / NaN.  topics / topic_sims may be NULL (no topics: untouched). */
int mvhdp_emb_nearest(mvhdp_handle h, const double* query /*[C]*/, int32_t n, int32_t* words, double* word_sims, int32_t* topics, double* topic_sims);
/* frees the embedding state (mvhdp_destroy and the exit handler do too); a mix that was set stands (it owns its table) */
int mvhdp_emb_release(mvhdp_handle h);

/* ---- useVectorsLambda: the sweep with the embeddings' p(w|t) mixed in, view 0 only (WRK:504-507, PTM:2673-2678, UPD:244-260):
 *     p_wt = lambda * (expDotProductValues[k][w] / sumExpValues[k]) + (1 - lambda) * ((n_wk + beta_0) / (n_k + betaSum_0))
 * in the document term of every view-0 token and in every leaf of a view-0 word tree (0 for an inactive topic, as ever).  Views m > 0,
 * modelLogLikelihood, the diagnostics, mvhdp_build_inference_trees, mvhdp_init_assignments_from_trees and MVHDP_SWEEP_FROZEN do not use it
 * (the inferencer's worker has lambda = 0, INF:251-252).  Nor do mvhdp_predict_items / mvhdp_score_items: their phi is the count term alone.
 * lambda == 0: mix off (the state after mvhdp_create: the kernels launched are those of a handle that never set one).  0 < lambda <= 1: on.
 * Anything else, NaN included: MVHDP_ERR_INVALID_ARG.  lambda is confined to [0, 1] because the samplers' certified prefix scan and their
 * fp32 screening rest on every term of the document sum being non-negative.
 * exp_dot [K][V_0] / sum_exp [K]: host arrays in the reference's layout, every entry finite, exp_dot >= 0, sum_exp > 0, every
 * lambda * (exp_dot / sum_exp) finite and within fp32's range (else MVHDP_ERR_INVALID_ARG, the mix in force untouched); or both NULL: the handle's own softmax table and accumulated sums as the last
 * mvhdp_emb_softmax left them (MVHDP_ERR_STATE when there is none).  The handle keeps lambda * (e / S) as a table of its own, [V_0][K] fp64,
 * and its fp32 rounding for the samplers' fp32 screening (12 V_0 K bytes: 240 MB at V_0 = 50 000, K = 400; mvhdp_destroy and
 * lambda = 0 free them): a later mvhdp_emb_softmax does NOT change what the samplers read until the next
 * mvhdp_set_vectors_mix (the reference switches at one point too, PTM:1199-1207).  Invalidates the F+trees (mvhdp_trees_current -> 0).
 * With a mix on:  deferred sweeps in every form (segments, ONLY_SEGMENT, NO_APPLY + mvhdp_apply_delta*, SEGMENT_APPLY, SEGMENT_OVERLAP,
 * mvhdp_sweep_many, inactive topics) sample with it, bit for bit what the sequential restatement tests/native/mix_ref.c gives;
 * MVHDP_SWEEP_LIVE runs in its stored-tree form only (mvhdp_tuning.live_rows is ignored: trees rebuilt with the mix at every segment border,
 * four segments by default; the 16-bit mirror form, live16, works as without a mix); a group's members each carry their own copy
 * (mvhdp_group_sweep: MVHDP_ERR_STATE when its local members disagree on lambda; across processes equality is the host's duty like the
 * flags'; MVHDP_SWEEP_ASYNC_EXCHANGE and MVHDP_SWEEP_SHARD_BIRTHS with a mix: MVHDP_ERR_UNSUPPORTED).
 * The walk-threshold search keeps a state of its own for sweeps with a mix; it is NOT persisted: mvhdp_get_tuning / mvhdp_set_tuning
 * report and restore the search of the sweeps without a mix only (learnt_walk_step[3] stays reserved), so a resumed chain with a mix
 * searches again. */
int mvhdp_set_vectors_mix(mvhdp_handle h, double lambda, const double* exp_dot /*[K][V_0] or NULL*/, const double* sum_exp /*[K] or NULL*/);
/* lambda (0: off) and, unless NULL, the table lambda * (e / S) as the device holds it, [V_0][K] (MVHDP_ERR_STATE when the mix is off).  Either may be NULL. */
int mvhdp_get_vectors_mix(mvhdp_handle h, double* lambda, double* mix /*[V_0][K] or NULL*/);

/* ---- the hot path ---- */
/* One Gibbs sweep over every entity: replaces "submit updaters + submit
 * workers + barrier.await()" PTM:1213-1239, i.e. WRK:186-233 x nst threads and
 * UPD:164-297 x nut threads.  sweep_idx and seed select the counter-based RNG
 * stream that stands in for ThreadLocalRandom (WRK:517,534).  p_override:
 * host [D][M][M] view weights drawn as WRK:327-337, or NULL to draw them on
 * the device (same nextBeta algorithm over a Philox stream).  dbg may be NULL.
 * Synchronous. */
int mvhdp_sweep(mvhdp_handle h, uint32_t sweep_idx, uint64_t seed, uint32_t flags,
                const double* p_override, const mvhdp_debug* dbg, mvhdp_sweep_stats* stats);
/* n sweeps, indices first_idx .. first_idx+n-1, enqueued back to back: the iteration loop PTM:1146-1239 without a host
 * round trip per iteration (one plan for the batch, statistics collected on the device, one synchronisation at the end).
 * Same integers as n calls of mvhdp_sweep with p_override = dbg = NULL.  stats: [n] or NULL (total_ms is the batch's time / n).
 * Falls back to n single calls where every sweep needs the host: a model with inactive topics (activation UPD:263-270),
 * MVHDP_SWEEP_NO_APPLY. */
int mvhdp_sweep_many(mvhdp_handle h, uint32_t first_idx, int32_t n, uint64_t seed, uint32_t flags, mvhdp_sweep_stats* stats /*[n]*/);
/* n_wk += delta, n_k += delta, delta = 0; also performs the topic activation
 * recorded by the sweep when (topic,modality) >= 0 (multi-GPU: the host passes
 * the winner of the min-reduction over activation_key). */
int mvhdp_apply_delta(mvhdp_handle h, int32_t activated_topic, int32_t activated_modality);
/* The same update as a stream-ordered pipeline, for document shards on several GPUs: the all-reduce of the delta buffer
 * can be issued in row-range chunks and each chunk's rows applied AND their F+trees rebuilt (buildFTrees PTM:2660-2696
 * from the updated counts) while the next chunk is still on the wire.  n_wk rows are numbered over all views (view m
 * starts at num_types[0] + .. + num_types[m-1]); the tokensPerTopic part sits behind the last row in both buffers.
 *   mvhdp_apply_delta_begin    applies the tokensPerTopic part (all-reduce it first: every tree needs all of it)
 *   mvhdp_apply_delta_rows     rows [row_begin, row_end): counts += delta, delta = 0, trees of those rows rebuilt; no wait
 *   mvhdp_apply_delta_end      every row must have been applied exactly once; topic activation as mvhdp_apply_delta;
 *                              one synchronisation; negative counts reported here
 * Afterwards mvhdp_trees_current() is 1 (unless a topic was activated) and the next sweep may pass REUSE_TREES. */
int mvhdp_apply_delta_begin(mvhdp_handle h);
int mvhdp_apply_delta_rows(mvhdp_handle h, int64_t row_begin, int64_t row_end);
int mvhdp_apply_delta_end(mvhdp_handle h, int32_t activated_topic, int32_t activated_modality);
/* The births of a MVHDP_SWEEP_SHARD_BIRTHS sweep over document shards (UPD:263-270: a topic leaves inActiveTopicIndex with the first
 * delta that reaches it; WRK:522-526: the samplers then draw the next inactive index).  get: a host copy of MVHDP_BUF_BIRTH_KEYS after a
 * NO_APPLY sweep.  activate: after mvhdp_apply_delta(h, -1, -1) or mvhdp_apply_delta_end(h, -1, -1), every topic k whose key is not
 * MVHDP_ACT_KEY_NONE is activated in index order -- alpha[view(key)][k] takes alpha[view(key)][K], k leaves inActiveTopicIndex -- and the
 * F+trees are invalidated if anything was born.  keys: [K] host memory (the MIN over all shards' tables), or NULL for MVHDP_BUF_BIRTH_KEYS
 * as it stands on the device.  The whole table is checked first: a key whose topic field is not its index, a view >= M, a key on an active
 * topic, or births that are not a prefix of the inactive topics in index order return MVHDP_ERR_INVALID_ARG with the model untouched. */
int mvhdp_get_birth_keys(mvhdp_handle h, int64_t* keys /*[K]*/);
int mvhdp_activate_births(mvhdp_handle h, const int64_t* keys /*[K] or NULL*/);
int mvhdp_trees_current(mvhdp_handle h);   /* 1: the F+trees match the counts and hyper-parameters, 0: not, < 0: error */
/* the per-document view weights used by the last sweep */
int mvhdp_get_view_weights(mvhdp_handle h, double* p /*[D][M][M]*/);

/* ---- tuning: the sweep's own choices, pinned or carried over ----
 * None of these changes a result: they decide which kernel variant visits an entity and when a word tree is walked, never
 * what is sampled.  The library reads the environment ONCE, in mvhdp_create (MVHDP_FORCE_RMAX, MVHDP_NARROW, MVHDP_LIVE16,
 * MVHDP_WALK_THETA, MVHDP_SINGLE_STREAM, MVHDP_PRIMARY_MIN_SHARE, MVHDP_LIVE_ROWS, MVHDP_DEBUG: diagnostics); a host uses this block.
 * learnt_walk_step / tree_branch_share are what the walk-threshold search has found: read them from one handle
 * (mvhdp_get_tuning) and hand them to another -- a document shard, a resumed chain -- and it does not search again. */
typedef struct {
    int32_t force_primary;                       /* 0: the library chooses; 1,2,4,8,16: primary register variant; 32: generic kernel only */
    int32_t narrow;                              /* -1: 16-bit mirror of n_wk wherever legal (default); 0: never; 1: for the 1-round kernel variant only; 2 (mvhdp_plan_probe only): as -1, and the probe plans for a handle that keeps the 12-bit image (views below 2^28 types); mvhdp_set_tuning takes 2 as -1: whether a handle keeps the image is decided at mvhdp_create */
    int32_t walk_fixed;                          /* 1: walk_theta[] as given, no search */
    int32_t single_stream;                       /* 1: all class kernels on the handle's stream (diagnostics) */
    int32_t live16;                              /* MVHDP_SWEEP_LIVE keeps the light n_wk rows current in the 16-bit mirror (half-width gathers): -1 where K >= 256 (default), 0 never, 1 always */
    int32_t single_wave;                         /* diagnostics, 0 by default.  1: every sweep kernel runs as ONE wavefront (one block of 64 threads), the class kernels one
                                                    after another, and a live sweep waits for its chunk-end atomics and drops its L1 before it goes on: a live sweep then IS
                                                    the sequential algorithm (every token sees every earlier update of the same segment), so the 32-bit form and the 16-bit
                                                    mirror form must give the same integers (tests/test_gpu_live.py) */
    double  walk_theta[MVHDP_MAX_MODALITIES];    /* with walk_fixed: walk a token's word tree up front iff u1 >= walk_theta[view] */
    double  primary_min_share;                   /* narrowest kernel class holding this share of the tokens gets its own kernel (0 = default 0.10) */
    int32_t learnt_walk_step[4];                 /* searched threshold in 1/20 steps per kernel flavour: [0] 1-round variant on the 16-bit mirror, [1] 1-round
                                                    variant on 32-bit rows, [2] the wider variants; -1: none yet (the library's default); [3] reserved */
    double  tree_branch_share[MVHDP_MAX_MODALITIES]; /* tree-branch (WRK:533) share of each view's tokens in the last measured sweep; < 0: not measured */
    int32_t live_overlap;                        /* MVHDP_SWEEP_LIVE with several segments: -1 (default) / 1: the next segment's trees are rebuilt (from the live counts)
                                                    and its kernels launched when the current segment is nearly through, so that no segment border idles the chip;
                                                    0: one segment after the other (the round-3 form) */
    int32_t live_rows;                           /* MVHDP_SWEEP_LIVE: -1 (default) / 1: the tree branch of a token (WRK:533-535) samples from the word's LIVE count row
                                                    (see MVHDP_SWEEP_LIVE) wherever every kernel of the sweep is register-resident; one segment per sweep by default;
                                                    0: stored trees rebuilt at every segment border, four segments by default (the round-4 form) */
} mvhdp_tuning;
int mvhdp_get_tuning(mvhdp_handle h, mvhdp_tuning* t);
int mvhdp_set_tuning(mvhdp_handle h, const mvhdp_tuning* t);

/* The sweep's planner and its walk-threshold search are pure functions (mvtopicmodel_amd/csrc/mvhdp_plan.h); these two run
 * them WITHOUT a device or a handle, on recorded inputs (tests/test_plan.py). */
typedef struct {
    int32_t num_topics, num_modalities;
    int64_t num_entities;
    int64_t max_entity_tokens;                   /* longest entity, all views together */
    int64_t entities_longer_than[5];             /* entities with more than 64, 128, 256, 512, 1024 tokens */
    uint64_t tokens_by_list_rounds[17];          /* tokens of the entities whose topic list needs 1..16, >16 rounds of 64 slots */
    uint64_t entities_by_class[8];               /* entities per kernel class 0..5 (64 << c slots; 5: generic kernel); [6]: list size not known */
    uint32_t flags;                              /* MVHDP_SWEEP_* */
    int32_t debug, batch, trees_current;
    int32_t num_cus;                             /* 0 = 256 */
    int32_t kernel_registers[6][3];              /* VGPRs of each kernel class: plain, walk flavour, debug build */
    int32_t inactive_topics;                     /* 1: inActiveTopicIndex is not empty (a live sweep then takes more segments: a topic is born per border) */
    int32_t vectors_mix;                         /* 1: a useVectorsLambda mix is set (mvhdp_set_vectors_mix): the mix flavours of the kernels run -- always the walk
                                                    flavour --, a live sweep takes its stored-tree form.  0: today's plans, bit for bit */
    int32_t kernel_registers_mix[6][3];          /* VGPRs of the mix flavours, as kernel_registers ([.][0] unused); a 0 takes the plain flavour's count */
    int32_t unassigned;                          /* 1: some token may still be unassigned (z = -1, a handle between mvhdp_set_corpus / mvhdp_set_assignments and its first
                                                    full sweep): row totals can grow, so no 16-bit delta cells and no live 16-bit mirror.  0: today's plans, bit for bit.
                                                    (Sits in what was the struct's tail padding: its size has not changed.) */
} mvhdp_plan_input;
typedef struct {
    int32_t status;                              /* what mvhdp_sweep would return for these flags (MVHDP_OK or an error) */
    int32_t segments, primary_class, register_resident, need_full_trees, dominant_class;
    int64_t routed_prefix;                       /* entities of the longest-first order that go through the route pass */
    int32_t class_used[6], class_map[6], class_stream[6], class_grid[6], class_walk[6], class_narrow[6], class_register_resident[6];
    int64_t class_lds_bytes[6];
    double  class_theta0[6];                     /* walk threshold of view 0 for that class's kernel */
    int32_t delta16, live_rows;                  /* delta16 1: the sweep keeps the n_wk deltas of rows with at most 32767 tokens in 16-bit cells (half the table the
                                                    chunk-end atomics land in), plain deferred sweeps only; live_rows 1: a live sweep in its live-rows form
                                                    (mvhdp_tuning.live_rows) */
} mvhdp_plan_output;
int mvhdp_plan_probe(const mvhdp_plan_input* in, const mvhdp_tuning* tuning /* or NULL */, mvhdp_plan_output* out);
/* The search alone: a kernel whose time per token at threshold step i is ns_by_step[i] (i = 0..20); steps_out[k] = the
 * threshold step proposed for sweep k. */
int mvhdp_tuner_probe(int32_t num_modalities, const double* tree_branch_share /*[M]*/, const double* u1_hist /*[20] or NULL*/,
                      const double* ns_by_step /*[21]*/, int32_t n_sweeps, int32_t group, int32_t* steps_out /*[n_sweeps]*/);

/* ---- the launch census: which compiled sweep kernel ran, over how many tokens (diagnostics; off by default, per handle) ----
 * The sweep is compiled 60 times -- the 56 instantiations of the register-resident kernel (rmax, debug, walk, narrow, roomy, liverows, mix:
 * its template arguments) and the four builds of the generic kernel (rmax = 0: debug, mix) -- and which of them a class launch gets is
 * decided by the planner, the tuning block and the environment.  With the census on, every class launch is counted where its kernel is looked
 * up (launches) and counts its statistics into a block of its own, which a small kernel behind the segment adds into the sweep's counters and,
 * by its tokens, into the row of that kernel (tokens: a launch over an empty queue counts as a launch and adds none).  Nothing a sweep
 * returns or leaves behind changes; with the census off nothing is allocated or enqueued for it.
 * enable: 1 on, 0 off, -1 leave as is; reset != 0 zeroes the tallies; rows: [cap] or NULL; *n_rows (may be NULL) = the rows that exist (60),
 * always in the same order. */
typedef struct { int32_t rmax /* 0: the generic kernel */, debug, walk, narrow, roomy, liverows, mix, reserved;
                 int64_t launches, tokens; } mvhdp_census_row;
int mvhdp_sweep_census(mvhdp_handle h, int32_t enable, int32_t reset, mvhdp_census_row* rows, int32_t cap, int32_t* n_rows);

/* ---- document shards on several GPUs: the exchange step inside the library ----
 * What the reference keeps inside its own process -- the nst x nut queue mesh between sampler and updater threads and the
 * barrier that ends an iteration (PTM:1042-1049, PTM:1232) -- for samplers that are GPUs: every member handle holds a
 * contiguous range of entities (mvhdp_config.doc_id_base = global id of its first entity) and a full replica of the model.
 * One mvhdp_group_sweep = every member samples its entities against the same snapshot; the int32 deltas are summed over all
 * members (on the device where members share a GPU, by RCCL all-reduce over xGMI between GPUs: the only collective of the
 * path), pipelined in row ranges with the update and F+tree rebuild of the rows that have arrived; with inactive topics the
 * activation key (MVHDP_ACT_KEY) is MIN-reduced so that every replica activates the same topic (UPD:263-270) -- or, with
 * MVHDP_SWEEP_SHARD_BIRTHS, the per-topic table of birth keys, so that every replica activates the same topics.  Results are
 * bit-identical to one handle holding every entity.  RCCL is opened at run time (a copy already mapped into the process, else the
 * file MVHDP_RCCL_LIB names, else librccl.so.1; MVHDP_RCCL_LIB_FIRST=1 tries the named file before a mapped copy -- tests): a single-GPU host never loads it.  A handle belongs to at most one group; destroy
 * the group before its members (a group call on a group whose member is gone returns MVHDP_ERR_STATE).  Group calls leave the
 * caller's current HIP device as they found it. */
typedef struct mvhdp_group_ctx* mvhdp_group;
#define MVHDP_UNIQUE_ID_BYTES 128
typedef struct {
    int32_t local_members;        /* handles of this process in the group */
    int32_t local_devices;        /* distinct GPUs among them = RCCL ranks of this process */
    int32_t ranks, first_rank;    /* RCCL ranks over all processes; rank of this process's first device */
    int32_t rccl;                 /* 1: the collective is RCCL; 0: one device and no RCCL installed (device-side sum only) */
    int32_t rccl_version;
    int32_t exchange_chunks;      /* row ranges per exchange (default 4) */
    int32_t exchange_packed;      /* 1: the n_wk deltas of the rows whose type holds at most 32767 tokens travel two to a 32-bit word (a delta of one sweep,
                                     summed over all ranks, cannot leave 16 bits there): agreed on by every rank behind the first completed sweep after a
                                     (re)count, 0 until then */
    double  last_exchange_ms;     /* device time of the last sweep's exchange on this process's first device: collectives + updates + tree rebuilds */
    int64_t last_exchange_bytes;  /* bytes this process handed to the collective in the last sweep, per device (96 MB at C4 at full width, 49 MB packed) */
} mvhdp_group_info;
/* one process drives n GPUs (the Java host of INTEGRATION.md): ncclCommInitAll over the members' devices */
int mvhdp_group_create(int32_t n, const mvhdp_handle* members, mvhdp_group* out);
/* one process per GPU: rank 0 obtains an id, the host's launcher hands it to every rank, every rank calls create_rank (collective) */
int mvhdp_group_unique_id(uint8_t* id /*[MVHDP_UNIQUE_ID_BYTES]*/);
int mvhdp_group_create_rank(mvhdp_handle member, const uint8_t* id /*[MVHDP_UNIQUE_ID_BYTES]*/, int32_t rank, int32_t nranks, mvhdp_group* out);
int mvhdp_group_destroy(mvhdp_group g);
const char* mvhdp_group_last_error(mvhdp_group g);           /* g may be NULL: last create error */
int mvhdp_group_get_info(mvhdp_group g, mvhdp_group_info* info);
int mvhdp_group_set_exchange_chunks(mvhdp_group g, int32_t chunks /* 1..64 */);
/* buildInitialTypeTopicCounts PTM:600-652 over all shards: every member counts its entities, the counts are summed over the group */
int mvhdp_group_build_counts(mvhdp_group g);
/* flags: MVHDP_SWEEP_LIVE (+ LIVE_SEGMENTS, + SHARD_BIRTHS), SEGMENT_APPLY (+ LIVE_SEGMENTS), EXACT_CHAIN, GENERIC_KERNEL; stats: one per
 * local member, or NULL.  Every rank passes the same flags (the collectives a step enters depend on them).
 * With LIVE | SHARD_BIRTHS and inactive topics every member gives birth chunk by chunk along the same list, the members' birth tables are
 * MIN-merged and MIN-all-reduced (K int64 instead of the one activation key) and every replica activates what any shard reached
 * (mvhdp_activate_births): births in index order, any number per exchange.  Births stay one per exchange in the deterministic modes.
 * Failure (one process per GPU): every rank enters the same collectives whatever happens locally; a rank whose sweep failed contributes
 * zero deltas and raises a status word that is reduced with the tokensPerTopic part, so ALL ranks return an error from the same call
 * (the failing rank its own, the others MVHDP_ERR_STATE) and none waits inside a collective for a rank that has given up.  After such
 * an error call mvhdp_group_build_counts on every rank (a recount from the assignments) before the next sweep. */
int mvhdp_group_sweep(mvhdp_group g, uint32_t sweep_idx, uint64_t seed, uint32_t flags, mvhdp_sweep_stats* stats);
/* The collective off the critical path, for LIVE sweeps of a group (opt-in).  A live sweep across shards is AD-LDA already: a replica
 * is live for its own entities and stale for the others'.  With this flag sweep t keeps its own changes in place, puts its deltas on
 * the wire at once -- the all-reduce runs on a stream of its own BESIDE sweep t+1 -- and the other shards' share of them is added when
 * sweep t+1 has been sampled: the step costs max(sampling, collective) instead of their sum, the chain sees the other shards' tokens
 * one to two sweeps late instead of zero to one.  Between such sweeps the replicas differ (each lacks the others' last sweep):
 * mvhdp_group_drain lands what is in flight and makes every replica the global model (the group's statistics, build_counts and any
 * sweep without the flag drain by themselves).  A failure shows one sweep late, on every rank together.  Not with inactive topics. */
#define MVHDP_SWEEP_ASYNC_EXCHANGE 0x100u
int mvhdp_group_drain(mvhdp_group g);
/* A host whose rank cannot go on calls this before its next mvhdp_group_sweep: that sweep samples nothing here and fails on every rank
 * together (see above) instead of leaving the others inside an all-reduce. */
int mvhdp_group_abort(mvhdp_group g);

/* ---- the steps either side of the sweep for a sharded model: what estimate() does every optimizeInterval and every tenth iteration
 * (PTM:1173-1210 -> optimizeP PTM:2698-2819, optimizeDP PTM:2440-2591, optimizeGamma PTM:2369-2438, optimizeBeta PTM:2288-2367;
 * PTM:1296-1320 -> modelLogLikelihood PTM:3322-3452).  Statistics over the replicated counts are any member's; statistics over the
 * entities are put together from the members -- in one process in ascending doc_id_base with the running sums carried from member to
 * member (the single handle's additions in the single handle's order: bit-identical), across processes by adding every rank's partial
 * result in rank order (equal to rounding; collective: every rank calls).  Arguments as for the single-handle functions. ---- */
int mvhdp_group_set_hyper(mvhdp_group g, const mvhdp_hyper* hy);          /* every local member (replicated: every rank passes the same values) */
/* mvhdp_remap_topics on every local member: each remaps its own entities' z and its replica of the counts, alpha and the inactive set.  The
 * counts are replicated, so nothing is exchanged; every rank passes the same map, as with mvhdp_group_set_hyper.  MVHDP_ERR_STATE, nothing
 * changed, unless the group is drained (no MVHDP_SWEEP_ASYNC_EXCHANGE in flight: mvhdp_group_drain) and not failed (no mvhdp_group_abort
 * raised, every member's counts current: mvhdp_group_build_counts after a failed sweep); every member is asked for its own refusals
 * before any of them remaps.  stats: moved and dropped summed over the local members; vacated and retired are those of the replicated model. */
int mvhdp_group_remap_topics(mvhdp_group g, const mvhdp_remap_args* a, mvhdp_remap_stats* stats /* or NULL */);
int mvhdp_group_log_likelihood(mvhdp_group g, double* log_likelihood /*[M]*/);
int mvhdp_group_doc_topic_hist(mvhdp_group g, int32_t m, int32_t* hist /*[K][hist_len]*/, int32_t hist_len,
                               int32_t* doc_len_counts /*[len_len]*/, int32_t len_len);
int mvhdp_group_count_histogram(mvhdp_group g, int32_t m, int32_t* hist, int32_t len);
int mvhdp_group_view_overlap_sums(mvhdp_group g, double* sums /*[M][M]*/);
int mvhdp_group_gamma_doc_statistics(mvhdp_group g, int32_t m, double gamma_m, uint64_t seed, uint32_t round, double* qs, double* qw);
/* mvhdp_diagnostics of the whole model.  Top words, typeDiscrWeight / discrWeightPerModality and the column reductions are statistics
 * of the replicated counts: any member's (so the group has no mvhdp_top_words / mvhdp_discr_weights of its own: call them on any
 * member).  The document pass runs on every member over its own entities; its integer accumulators are summed over the group, the
 * per-topic sums of c log c added member by member (ascending doc_id_base) and rank by rank.  Collective across processes. */
int mvhdp_group_diagnostics(mvhdp_group g, const mvhdp_diag_args* args, mvhdp_diag_out* out);

/* ---- interop for collectives and stream sharing ---- */
int mvhdp_device_buffer(mvhdp_handle h, mvhdp_buffer which, void** dev_ptr, size_t* bytes);
/* The caller has written MVHDP_BUF_COUNTS through the device pointer (e.g. the all-reduce of the shards' initial
 * counts): the counts are now valid, any F+trees built from the old values are not. */
int mvhdp_counts_written(mvhdp_handle h);
int mvhdp_set_stream(mvhdp_handle h, void* hip_stream /* hipStream_t, NULL = library's own */);
int mvhdp_synchronize(mvhdp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* MVHDP_H */
