/* fake_mvhdp.c -- a stand-in for libmvhdp.so on the CPU side of the JNI tests (tests/test_jni_fake_jvm.py).  A handle cannot exist
 * without a device, so the shim's lifecycle and refusal paths are run against this instead: it exports every mvhdp_* symbol the shim
 * imports, logs every call by name, and does nothing else -- except for a handful that record what they were handed (create, destroy,
 * set_corpus, get_counts, top_words, sweep, sweep_many, get_tuning, set_tuning, group_create, group_destroy, last_error) and the four
 * post-training calls whose scalar outputs the shim reads back (similar_pairs, doc_topics_top, topic_phrases, heldout_left_to_right: on
 * MVHDP_OK a recognisable value in each, within the capacities handed in).  Every other function is one line:
 * it returns the status fm_set_status() chose (MVHDP_ERR_UNSUPPORTED unless told otherwise) and touches none of its pointers.
 * mvhdp_sweep_many and mvhdp_heldout_left_to_right can be made to block until the test lets them go.  It is NOT a second implementation
 * of anything. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "mvhdp.h"

#define EXPORT __attribute__((visibility("default")))
#define LOG_MAX 8192

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_cv = PTHREAD_COND_INITIALIZER;
static const char* g_log[LOG_MAX];
static int g_log_len;
static int g_status = MVHDP_ERR_UNSUPPORTED;
static int g_block_sweeps, g_sweeps_inside, g_sweeps_returned;

static struct {
    mvhdp_config create_cfg;
    int creates, destroys, group_creates, group_destroys;
    void* destroyed[64];
    int corpus_m; int64_t corpus_docs, corpus_last_off; int32_t corpus_first_token; int corpus_tokens_null;
    uint32_t sweep_idx, sweep_flags; uint64_t sweep_seed; int sweep_has_p; double sweep_p0, sweep_p_last; int sweep_n;
    mvhdp_tuning given_tuning;
    int group_n; void* group_members[64];
    int top_m, top_n;
} g_rec;

/* begin() logs the call and returns the status to answer with; it HOLDS g_mu until end(), so that whatever a function records in g_rec
 * in between is written under the mutex the fm_* readers take (the race tests call in from several threads) */
static int begin(const char* name)
{
    pthread_mutex_lock(&g_mu);
    if (g_log_len < LOG_MAX) g_log[g_log_len++] = name;
    return g_status;
}
static int end(int rc) { pthread_mutex_unlock(&g_mu); return rc; }
static int logged(const char* name) { return end(begin(name)); }

/* ---- what the test drives ---- */
EXPORT void fm_reset(void) { pthread_mutex_lock(&g_mu); g_log_len = 0; g_status = MVHDP_ERR_UNSUPPORTED; memset(&g_rec, 0, sizeof g_rec); g_sweeps_returned = 0; pthread_mutex_unlock(&g_mu); }
EXPORT void fm_set_status(int rc) { pthread_mutex_lock(&g_mu); g_status = rc; pthread_mutex_unlock(&g_mu); }
EXPORT int fm_log_len(void) { pthread_mutex_lock(&g_mu); int n = g_log_len; pthread_mutex_unlock(&g_mu); return n; }
EXPORT const char* fm_log_at(int i) { pthread_mutex_lock(&g_mu); const char* s = i >= 0 && i < g_log_len ? g_log[i] : ""; pthread_mutex_unlock(&g_mu); return s; }
EXPORT void fm_block_sweeps(int on) { pthread_mutex_lock(&g_mu); g_block_sweeps = on; pthread_cond_broadcast(&g_cv); pthread_mutex_unlock(&g_mu); }
EXPORT int fm_sweeps_inside(void) { pthread_mutex_lock(&g_mu); int n = g_sweeps_inside; pthread_mutex_unlock(&g_mu); return n; }
EXPORT int fm_sweeps_returned(void) { pthread_mutex_lock(&g_mu); int n = g_sweeps_returned; pthread_mutex_unlock(&g_mu); return n; }
static int counter(const char* what)
{
    if (!strcmp(what, "creates")) return g_rec.creates;
    if (!strcmp(what, "destroys")) return g_rec.destroys;
    if (!strcmp(what, "group_creates")) return g_rec.group_creates;
    if (!strcmp(what, "group_destroys")) return g_rec.group_destroys;
    if (!strcmp(what, "group_n")) return g_rec.group_n;
    if (!strcmp(what, "corpus_m")) return g_rec.corpus_m;
    if (!strcmp(what, "corpus_tokens_null")) return g_rec.corpus_tokens_null;
    if (!strcmp(what, "sweep_has_p")) return g_rec.sweep_has_p;
    if (!strcmp(what, "sweep_n")) return g_rec.sweep_n;
    if (!strcmp(what, "top_m")) return g_rec.top_m;
    if (!strcmp(what, "top_n")) return g_rec.top_n;
    return -12345;
}
#define LOCKED(...) do { pthread_mutex_lock(&g_mu); __VA_ARGS__; pthread_mutex_unlock(&g_mu); } while (0)
EXPORT int fm_counter(const char* what) { int v; LOCKED(v = counter(what)); return v; }
EXPORT void fm_create_config(mvhdp_config* out) { LOCKED(*out = g_rec.create_cfg); }
EXPORT void fm_corpus(int64_t* out) { LOCKED(out[0] = g_rec.corpus_docs; out[1] = g_rec.corpus_last_off; out[2] = g_rec.corpus_first_token); }
EXPORT void fm_sweep_args(int64_t* out, double* p) { LOCKED(out[0] = g_rec.sweep_idx; out[1] = (int64_t)g_rec.sweep_seed; out[2] = g_rec.sweep_flags; p[0] = g_rec.sweep_p0; p[1] = g_rec.sweep_p_last); }
EXPORT void* fm_group_member(int i) { void* v; LOCKED(v = g_rec.group_members[i]); return v; }
EXPORT void* fm_destroyed(int i) { void* v; LOCKED(v = g_rec.destroyed[i]); return v; }
EXPORT int fm_tuning_size(void) { return (int)sizeof(mvhdp_tuning); }
EXPORT void fm_given_tuning(mvhdp_tuning* out) { LOCKED(*out = g_rec.given_tuning); }

/* the tuning block mvhdp_get_tuning hands out: no field holds its default or a neighbour's value */
EXPORT void fm_made_tuning(mvhdp_tuning* t)
{
    memset(t, 0, sizeof *t);
    t->force_primary = 4; t->narrow = 1; t->walk_fixed = 1; t->single_stream = 1; t->live16 = 1; t->single_wave = 1;
    for (int m = 0; m < MVHDP_MAX_MODALITIES; m++) { t->walk_theta[m] = 0.125 + m; t->tree_branch_share[m] = 0.0625 * (m + 1); }
    t->primary_min_share = 0.375;
    t->learnt_walk_step[0] = 3; t->learnt_walk_step[1] = 7; t->learnt_walk_step[2] = 11; t->learnt_walk_step[3] = 13;
    t->live_overlap = 1; t->live_rows = 1;
}

/* statistics with a different value in every field of every sweep */
static void made_stats(mvhdp_sweep_stats* st, int i)
{
    memset(st, 0, sizeof *st);
    const int64_t b = 1000 * (int64_t)(i + 1);
    st->tokens = b + 1; st->changed = b + 2; st->new_mass_cnt = b + 3; st->topic_doc_mass_cnt = b + 4; st->word_ftree_mass_cnt = b + 5;
    st->oov_skipped = b + 6; st->aborted_docs = b + 7; st->exact_fallbacks = b + 8; st->activated_topic = (int32_t)b + 9;
    st->activated_modality = (int32_t)b + 10; st->activation_key = b + 11; st->sweep_kernel_ms = (double)b + 12.5; st->total_ms = (double)b + 13.5;
    st->activations = (int32_t)b + 14;
}

/* between begin() and end(): the call stays inside for as long as fm_block_sweeps(1) holds */
static void gate(void)
{
    g_sweeps_inside++;
    while (g_block_sweeps) pthread_cond_wait(&g_cv, &g_mu);       /* (gives g_mu up while it waits) */
    g_sweeps_inside--;
    g_sweeps_returned++;
}

/* ---- the ones that record ---- */
EXPORT int mvhdp_create(const mvhdp_config* cfg, mvhdp_handle* out)
{
    int rc = begin("mvhdp_create");
    g_rec.create_cfg = *cfg; g_rec.creates++;
    if (rc == MVHDP_OK) *out = (mvhdp_handle)malloc(16);
    return end(rc);
}
EXPORT int mvhdp_destroy(mvhdp_handle h)
{
    begin("mvhdp_destroy");
    if (g_rec.destroys < 64) g_rec.destroyed[g_rec.destroys] = h;
    g_rec.destroys++;
    end(MVHDP_OK);
    free(h);
    return MVHDP_OK;
}
EXPORT const char* mvhdp_last_error(mvhdp_handle h) { (void)h; logged("mvhdp_last_error"); return "the stand-in's message"; }
EXPORT const char* mvhdp_group_last_error(mvhdp_group g) { (void)g; logged("mvhdp_group_last_error"); return "the stand-in's group message"; }
EXPORT int mvhdp_set_corpus(mvhdp_handle h, int32_t m, int64_t num_docs, const int64_t* doc_off, const int32_t* tokens)
{
    (void)h;
    int rc = begin("mvhdp_set_corpus");
    g_rec.corpus_m = m; g_rec.corpus_docs = num_docs; g_rec.corpus_last_off = doc_off[num_docs];
    g_rec.corpus_tokens_null = tokens == NULL; g_rec.corpus_first_token = tokens ? tokens[0] : -1;
    return end(rc);
}
EXPORT int mvhdp_sweep(mvhdp_handle h, uint32_t sweep_idx, uint64_t seed, uint32_t flags, const double* p, const mvhdp_debug* dbg, mvhdp_sweep_stats* stats)
{
    (void)h; (void)dbg;
    int rc = begin("mvhdp_sweep");
    g_rec.sweep_idx = sweep_idx; g_rec.sweep_seed = seed; g_rec.sweep_flags = flags; g_rec.sweep_has_p = p != NULL;
    g_rec.sweep_p0 = p ? p[0] : 0.0; g_rec.sweep_n = 1;
    if (rc == MVHDP_OK) made_stats(stats, (int)sweep_idx);
    return end(rc);
}
EXPORT int mvhdp_sweep_many(mvhdp_handle h, uint32_t first_idx, int32_t n, uint64_t seed, uint32_t flags, mvhdp_sweep_stats* stats)
{
    (void)h;
    int rc = begin("mvhdp_sweep_many");
    g_rec.sweep_idx = first_idx; g_rec.sweep_seed = seed; g_rec.sweep_flags = flags; g_rec.sweep_n = n;
    gate();
    end(rc);
    if (rc == MVHDP_OK) for (int i = 0; i < n; i++) made_stats(&stats[i], (int)first_idx + i);
    return rc;
}
EXPORT int mvhdp_get_tuning(mvhdp_handle h, mvhdp_tuning* t) { (void)h; int rc = logged("mvhdp_get_tuning"); if (rc == MVHDP_OK) fm_made_tuning(t); return rc; }
EXPORT int mvhdp_set_tuning(mvhdp_handle h, const mvhdp_tuning* t) { (void)h; int rc = begin("mvhdp_set_tuning"); g_rec.given_tuning = *t; return end(rc); }
EXPORT int mvhdp_group_create(int32_t n, const mvhdp_handle* members, mvhdp_group* out)
{
    int rc = begin("mvhdp_group_create");
    g_rec.group_creates++; g_rec.group_n = n;
    for (int i = 0; i < n && i < 64; i++) g_rec.group_members[i] = members[i];
    if (rc == MVHDP_OK) *out = (mvhdp_group)malloc(16);
    return end(rc);
}
EXPORT int mvhdp_group_destroy(mvhdp_group g) { begin("mvhdp_group_destroy"); g_rec.group_destroys++; end(MVHDP_OK); free(g); return MVHDP_OK; }

/* (two outputs and two scalars, so that a release mode or an argument order gone wrong shows without a device) */
EXPORT int mvhdp_get_counts(mvhdp_handle h, int32_t m, int32_t* n_wk, int32_t* n_k)
{
    (void)h; (void)m;
    int rc = logged("mvhdp_get_counts");
    if (rc == MVHDP_OK && n_wk) n_wk[0] = 41;
    if (rc == MVHDP_OK && n_k) n_k[0] = 43;
    return rc;
}
EXPORT int mvhdp_top_words(mvhdp_handle h, int32_t m, int32_t n, int32_t* types, int32_t* counts, int32_t* nonzero)
{
    (void)h; (void)types; (void)counts; (void)nonzero;
    int rc = begin("mvhdp_top_words");
    g_rec.top_m = m; g_rec.top_n = n;
    return end(rc);
}

/* ---- the post-training calls: the scalars the shim reads back, never more than the capacity it passed ---- */
static int64_t at_most(int64_t cap, int64_t v) { return cap < v ? cap : v; }
EXPORT int mvhdp_similar_pairs(mvhdp_handle h, const mvhdp_sim_args* a, int64_t cap, int32_t* i, int32_t* j, double* sim, int64_t* count, mvhdp_sim_stats* stats)
{
    (void)h; (void)a; (void)i; (void)j; (void)sim;
    int rc = logged("mvhdp_similar_pairs");
    if (rc != MVHDP_OK) return rc;
    *count = at_most(cap, 3);
    if (stats) { stats->pairs_screened = 101; stats->candidates = 102; stats->emitted = 103; stats->stripes = 104; stats->regrown = 105; stats->margin = 0.625; }
    return rc;
}
EXPORT int mvhdp_doc_topics_top(mvhdp_handle h, const double* view_weights, int64_t d0, int64_t d1, double threshold, int32_t max, int64_t cap, int64_t* row_off,
                                int32_t* topics, double* weights, int64_t* count)
{
    (void)h; (void)view_weights; (void)d0; (void)d1; (void)threshold; (void)max; (void)row_off; (void)topics; (void)weights;
    int rc = logged("mvhdp_doc_topics_top");
    if (rc == MVHDP_OK) *count = at_most(cap, 2);
    return rc;
}
EXPORT int mvhdp_topic_phrases(mvhdp_handle h, const mvhdp_phrase_args* a, int64_t cap_phrases, int64_t cap_words, int64_t* topic_off, int64_t* word_off, int32_t* words,
                               int32_t* counts, int64_t* distinct, int64_t* occurrences, int64_t* n_phrases, int64_t* n_words, mvhdp_phrase_stats* stats)
{
    (void)h; (void)a; (void)topic_off; (void)word_off; (void)words; (void)counts; (void)distinct; (void)occurrences;
    int rc = logged("mvhdp_topic_phrases");
    if (rc != MVHDP_OK) return rc;
    *n_phrases = at_most(cap_phrases, 3); *n_words = at_most(cap_words, 5);
    if (stats) { stats->runs = 201; stats->occurrences = 202; stats->distinct = 203; stats->kept = 204; stats->hash_collisions = 205; }
    return rc;
}
EXPORT int mvhdp_heldout_left_to_right(mvhdp_handle h, const mvhdp_heldout_args* a, int64_t num_docs, const int64_t* doc_off, const int32_t* tokens, double* doc_ll,
                                       double* position_sum, int64_t* doc_tokens, mvhdp_heldout_stats* stats)
{
    (void)h; (void)a; (void)num_docs; (void)doc_off; (void)tokens; (void)doc_ll; (void)position_sum; (void)doc_tokens;
    int rc = begin("mvhdp_heldout_left_to_right");
    gate();
    end(rc);
    if (rc == MVHDP_OK && stats) { stats->log_likelihood = -12.5; stats->tokens = 301; stats->oov = 302; stats->visits = 303; }
    return rc;
}

/* ---- the one-liners ---- */
#define STUB(name, ...) EXPORT int name(__VA_ARGS__) { return logged(#name); }
STUB(mvhdp_set_assignments, mvhdp_handle h, int32_t m, const int32_t* z)
STUB(mvhdp_set_view_presence, mvhdp_handle h, int32_t m, const uint8_t* present)
STUB(mvhdp_get_assignments, mvhdp_handle h, int32_t m, int32_t* z)
STUB(mvhdp_set_hyper, mvhdp_handle h, const mvhdp_hyper* hy)
STUB(mvhdp_get_alpha, mvhdp_handle h, double* alpha, uint8_t* inactive)
STUB(mvhdp_build_counts, mvhdp_handle h)
STUB(mvhdp_build_trees, mvhdp_handle h)
STUB(mvhdp_get_doc_topic_hist, mvhdp_handle h, int32_t m, int32_t* hist, int32_t hist_len, int32_t* doc_len_counts, int32_t len_len)
STUB(mvhdp_get_count_histogram, mvhdp_handle h, int32_t m, int32_t* hist, int32_t len)
STUB(mvhdp_view_overlap_sums, mvhdp_handle h, double* sums)
STUB(mvhdp_model_log_likelihood, mvhdp_handle h, double* ll)
STUB(mvhdp_gamma_doc_statistics, mvhdp_handle h, int32_t m, double gamma_m, uint64_t seed, uint32_t round, double* qs, double* qw)
STUB(mvhdp_dp_table_statistics, mvhdp_handle h, int32_t m, const int32_t* hist, int32_t hist_len, const double* conc, uint64_t seed, uint32_t round, double* mk, uint8_t* active)
STUB(mvhdp_discr_weights, mvhdp_handle h, double* per_view, int32_t m, double* type_weight)
STUB(mvhdp_diagnostics, mvhdp_handle h, const mvhdp_diag_args* args, mvhdp_diag_out* out)
STUB(mvhdp_emb_init, mvhdp_handle h, const mvhdp_emb_config* cfg, const double* weights, uint64_t seed)
STUB(mvhdp_emb_count_words, mvhdp_handle h)
STUB(mvhdp_emb_train, mvhdp_handle h, int32_t epochs, uint64_t seed, uint32_t round, uint32_t flags, mvhdp_emb_stats* stats)
STUB(mvhdp_emb_get_vectors, mvhdp_handle h, double* weights, double* negative_weights)
STUB(mvhdp_emb_set_vectors, mvhdp_handle h, const double* weights, const double* negative_weights)
STUB(mvhdp_emb_word_stats, mvhdp_handle h, int64_t* counts, double* retention, int64_t* total_words)
STUB(mvhdp_emb_sampling_table, mvhdp_handle h, int64_t first, int64_t n, int32_t* types)
STUB(mvhdp_emb_softmax, mvhdp_handle h, int32_t reset_sums, double* exp_dot, double* sum_exp)
STUB(mvhdp_emb_nearest, mvhdp_handle h, const double* query, int32_t n, int32_t* words, double* word_sims, int32_t* topics, double* topic_sims)
STUB(mvhdp_emb_release, mvhdp_handle h)
STUB(mvhdp_set_vectors_mix, mvhdp_handle h, double lambda, const double* exp_dot, const double* sum_exp)
STUB(mvhdp_get_vectors_mix, mvhdp_handle h, double* lambda, double* mix)
STUB(mvhdp_entity_topic_distributions, mvhdp_handle h, const double* view_weights, double threshold, int32_t max, int32_t round_digits, int64_t n_groups,
     const int64_t* member_off, const int64_t* members, double* out)
STUB(mvhdp_apply_delta, mvhdp_handle h, int32_t activated_topic, int32_t activated_modality)
STUB(mvhdp_group_unique_id, uint8_t* id)
STUB(mvhdp_group_create_rank, mvhdp_handle member, const uint8_t* id, int32_t rank, int32_t nranks, mvhdp_group* out)
STUB(mvhdp_group_get_info, mvhdp_group g, mvhdp_group_info* info)
STUB(mvhdp_group_build_counts, mvhdp_group g)
STUB(mvhdp_group_sweep, mvhdp_group g, uint32_t sweep_idx, uint64_t seed, uint32_t flags, mvhdp_sweep_stats* stats)
STUB(mvhdp_group_drain, mvhdp_group g)
STUB(mvhdp_group_abort, mvhdp_group g)
STUB(mvhdp_group_log_likelihood, mvhdp_group g, double* ll)
STUB(mvhdp_group_doc_topic_hist, mvhdp_group g, int32_t m, int32_t* hist, int32_t hist_len, int32_t* doc_len_counts, int32_t len_len)
STUB(mvhdp_group_count_histogram, mvhdp_group g, int32_t m, int32_t* hist, int32_t len)
STUB(mvhdp_group_view_overlap_sums, mvhdp_group g, double* sums)
STUB(mvhdp_group_gamma_doc_statistics, mvhdp_group g, int32_t m, double gamma_m, uint64_t seed, uint32_t round, double* qs, double* qw)
STUB(mvhdp_group_diagnostics, mvhdp_group g, const mvhdp_diag_args* args, mvhdp_diag_out* out)
