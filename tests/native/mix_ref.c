/* mix_ref.c -- TEST INFRASTRUCTURE: the deferred sweep with the useVectorsLambda mix of view 0, restated sequentially in plain C.
 *
 * The CPU oracle (oracle/mvhdp_oracle.c) restates the reference with useVectorsLambda == 0 only (its orc_build_trees says so).  This
 * file restates the same three pieces WITH the mix, on the oracle's own model object and primitives (orc_token_uniforms,
 * orc_draw_p_philox, orc_ftree_construct / _sample, orc_lower_bound: linked from the oracle's library, not restated):
 *
 *   mxr_build_trees   FastQMVWVParallelTopicModel.buildFTrees            PTM:2660-2696 with the three-way p_wt of PTM:2673-2678
 *   mxr_sweep         FastQMVWVWorkerRunnable.sampleTopicsForOneDoc      WRK:301-601 with the document term of WRK:504-507,
 *                     FTree.sample FT:111-136 and the binary search WRK:257-277 through the oracle's primitives,
 *                     then FastQMVWVUpdaterRunnable's deferred apply and topic activation UPD:181-272
 *
 * In view 0 (`m == 0`, WRK:504, PTM:2673) with the mix on
 *     p_wt = lambda * (expDotProductValues[k][w] / sumExpValues[k]) + (1 - lambda) * ((n_wk + beta_0) / (n_k + betaSum_0))
 * The first product is formed once per (w, k) by mxr_make_mix -- a division, then the multiplication, as the reference writes them --
 * into a table [V_0][K]; `oml` = 1 - lambda is one double.  The updater's refresh of the two touched leaves (UPD:244-260) is what a
 * rebuild from the counts reproduces (the trees are rebuilt at the next sweep start, as in the oracle).
 * use_mix == 0 is the oracle's arithmetic, expression for expression: the tests pin this file to the oracle there.
 * Compile without contraction (-ffp-contract=off, no -ffast-math): Java never fuses a * b + c. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../oracle/mvhdp_oracle_internal.h"

#define MXR_REUSE_TREES 1u
#define MXR_NO_APPLY 2u
#define MXR_FROZEN 16u
/* The traced conditional of a listed topic is leaf / total + (its document term) / total.  The oracle and the generic LDS kernel take the
 * term as the difference of two running sums (the default here: what pins this file to the oracle); the register-resident kernels as
 * the product itself (p_mm n + other) p_wt.  With this flag the product is used: under the sequential sum (MVHDP_SWEEP_EXACT_CHAIN)
 * those kernels' traces are then these bit for bit. */
#define MXR_TRACE_PRODUCT 0x100u

/* mix[w][k] = lambda * (e[k][w] / S[k]); e in the reference's layout [K][V0] */
void mxr_make_mix(int V0, int K, double lambda, const double* e, const double* S, double* mix)
{
    for (int w = 0; w < V0; w++)
        for (int k = 0; k < K; k++) mix[(size_t)w * K + k] = lambda * (e[(size_t)k * V0 + w] / S[k]);
}

static inline double p_wt_of(const orc_model* o, int m, int cnt, int topic, int use_mix, const double* mixrow, double oml)
{
    const int K = o->K;
    if (use_mix && m == 0)                                                                        /* WRK:504-505, PTM:2673-2674 */
        return mixrow[topic] + oml * ((cnt + o->beta[m]) / (o->nk[(size_t)m * K + topic] + o->beta_sum[m]));
    return (cnt + o->beta[m]) / (o->nk[(size_t)m * K + topic] + o->beta_sum[m]);                  /* WRK:507, PTM:2676 */
}

void mxr_build_trees(orc_model* o, int use_mix, const double* mix, double oml)
{
    /* PTM:2660-2696 */
    const int K = o->K, M = o->M;
    double* temp = (double*)malloc((size_t)K * sizeof(double));
    int any_inactive = 0;
    for (int k = 0; k < K; k++) any_inactive |= o->inactive[k];
    for (int m = 0; m < M; m++)
        for (int w = 0; w < o->V[m]; ++w) {
            const int32_t* cnt = o->nwk + (size_t)(o->rowbase[m] + w) * K;
            const double* mixrow = (use_mix && m == 0) ? mix + (size_t)w * K : NULL;
            for (int t = 0; t < K; t++) {
                if (any_inactive && o->inactive[t]) temp[t] = 0;                                   /* PTM:2670-2671 */
                else temp[t] = o->gamma[m] * o->alpha[(size_t)m * (K + 1) + t] * p_wt_of(o, m, cnt[t], t, use_mix, mixrow, oml);   /* PTM:2678 */
            }
            orc_ftree_construct(o->trees + (size_t)(o->rowbase[m] + w) * 2 * K, K, temp);
        }
    free(temp);
}

typedef struct { int32_t oldT, newT, type, mod; int64_t key; } mxr_delta;        /* QD:12-36 */
typedef struct { mxr_delta* v; size_t n, cap; } mxr_dvec;

static void dv_push(mxr_dvec* dv, mxr_delta d)
{
    if (dv->n == dv->cap) { dv->cap = dv->cap ? 2 * dv->cap : 1024; dv->v = (mxr_delta*)realloc(dv->v, dv->cap * sizeof(mxr_delta)); }
    dv->v[dv->n++] = d;
}

/* WRK:301-601 for one entity against the snapshot (n_wk, n_k, trees); 1 if the Java would have thrown inside the entity */
static int sample_one_doc(orc_model* o, int use_mix, const double* mix, double oml, int64_t d, int64_t doc_global, uint32_t sweep, uint64_t seed,
                          const double* p, int first_inactive, orc_stats* st, mxr_dvec* dv, double* const* tok_dbg,
                          int n_trace, const int64_t* trace_doc, const int32_t* trace_view, const int32_t* trace_pos, double* trace_out,
                          int trace_product, double* terms,
                          int32_t* localTopicCounts, int32_t* localTopicIndex, double* topicDocWordMasses, double* totalMassOtherModalities)
{
    const int K = o->K, M = o->M;
    int docLength[ORC_MAX_M];
    memset(localTopicCounts, 0, (size_t)M * K * sizeof(int32_t));
    for (int m = 0; m < M; m++) {                                                                  /* WRK:327-361 */
        docLength[m] = 0;
        if (!o->doc_off[m]) continue;
        const int64_t b = o->doc_off[m][d], e = o->doc_off[m][d + 1];
        docLength[m] = (int)(e - b);
        for (int64_t i = b; i < e; i++) if (o->z[m][i] != -1) localTopicCounts[(size_t)m * K + o->z[m][i]]++;
    }
    int nonZeroTopics = 0;                                                                         /* WRK:376-391 */
    for (int topic = 0; topic < K; topic++)
        for (int i = 0; i < M; i++)
            if (localTopicCounts[(size_t)i * K + topic] != 0) { localTopicIndex[nonZeroTopics++] = topic; break; }

    for (int m = 0; m < M; m++) {                                                                  /* WRK:393 */
        const double scale = docLength[m] + (double)o->gamma[m] * o->alpha_sum[m];
        for (int k = 0; k < K; k++) totalMassOtherModalities[k] = 0;                               /* WRK:395 */
        for (int di = 0; di < nonZeroTopics; di++) {                                               /* WRK:399-410 */
            const int topic = localTopicIndex[di];
            for (int i = 0; i < M; i++)
                if (i != m && docLength[i] != 0)
                    totalMassOtherModalities[topic] += p[m * M + i]
                        * (localTopicCounts[(size_t)i * K + topic] + o->gamma[i] * o->alpha[(size_t)i * (K + 1) + topic])
                        / (docLength[i] + (double)o->gamma[i] * o->alpha_sum[i]);
            totalMassOtherModalities[topic] = totalMassOtherModalities[topic] * scale;
        }
        double newTopicMassAllModalities = 0;                                                      /* WRK:413-418 */
        for (int i = 0; i < M; i++)
            newTopicMassAllModalities += p[m * M + i] * (o->gamma[i] * o->alpha[(size_t)i * (K + 1) + K])
                / (docLength[i] + (double)o->gamma[i] * o->alpha_sum[i]);
        newTopicMassAllModalities = newTopicMassAllModalities * scale;

        if (docLength[m] == 0) continue;
        const int64_t base = o->doc_off[m][d];
        for (int position = 0; position < docLength[m]; position++) {                              /* WRK:425 */
            const int type = o->tokens[m][base + position];
            if (type >= o->V[m]) { st->oov_skipped++; continue; }                                  /* WRK:427-428 */
            const int oldTopic = o->z[m][base + position];
            const int32_t* currentTypeTopicCounts = o->nwk + (size_t)(o->rowbase[m] + type) * K;
            const double* currentTree = o->trees + (size_t)(o->rowbase[m] + type) * 2 * K;
            const double* mixrow = (use_mix && m == 0) ? mix + (size_t)type * K : NULL;

            if (oldTopic != -1) {                                                                  /* WRK:434-471 */
                localTopicCounts[(size_t)m * K + oldTopic]--;
                int gone = localTopicCounts[(size_t)m * K + oldTopic] == 0;
                for (int j = 0; gone && j < M; j++) gone = localTopicCounts[(size_t)j * K + oldTopic] == 0;
                if (gone) {
                    int di = 0;
                    while (localTopicIndex[di] != oldTopic) { di++; if (di >= K) return 1; }       /* ArrayIndexOutOfBounds */
                    while (di < nonZeroTopics) { if (di < K - 1) localTopicIndex[di] = localTopicIndex[di + 1]; di++; }
                    nonZeroTopics--;
                }
            }

            double topicDocWordMass = 0.0;                                                         /* WRK:496-513 */
            for (int di = 0; di < nonZeroTopics; di++) {
                const int topic = localTopicIndex[di];
                const int n = localTopicCounts[(size_t)m * K + topic];
                const double p_wt = p_wt_of(o, m, currentTypeTopicCounts[topic], topic, use_mix, mixrow, oml);   /* WRK:504-507 */
                terms[di] = (p[m * M + m] * n + totalMassOtherModalities[topic]) * p_wt;
                topicDocWordMass += terms[di];                                                     /* WRK:509 */
                topicDocWordMasses[di] = topicDocWordMass;
            }
            const double newTopicMass = (first_inactive < 0) ? 0 : newTopicMassAllModalities / K;  /* WRK:515 */

            double nextUniform, nextUniform2;
            orc_token_uniforms(seed, sweep, doc_global, m, (uint32_t)position, &nextUniform, &nextUniform2);
            double sample = nextUniform * (newTopicMass + topicDocWordMass + currentTree[1]);      /* WRK:519 */

            if (tok_dbg && tok_dbg[m]) {
                double* g = tok_dbg[m] + (size_t)(base + position) * 4;
                g[0] = newTopicMass; g[1] = topicDocWordMass; g[2] = currentTree[1]; g[3] = sample;
            }
            for (int t = 0; t < n_trace; t++)
                if (trace_doc[t] == d && trace_view[t] == m && trace_pos[t] == position) {
                    /* the full conditional: leaf_k / total, plus the slot terms, slot K = the new-topic mass */
                    double* out = trace_out + (size_t)t * (K + 1);
                    const double tot = newTopicMass + topicDocWordMass + currentTree[1];
                    for (int k = 0; k < K; k++) out[k] = currentTree[K + k] / tot;
                    double prev = 0;
                    for (int di = 0; di < nonZeroTopics; di++) {
                        out[localTopicIndex[di]] += (trace_product ? terms[di] : topicDocWordMasses[di] - prev) / tot;
                        prev = topicDocWordMasses[di];
                    }
                    out[K] = newTopicMass / tot;
                }

            int newTopic = -1;
            if (sample < newTopicMass) {                                                           /* WRK:522-526 */
                st->new_mass_cnt++;
                newTopic = first_inactive;
            } else {
                sample -= newTopicMass;
                if (sample < topicDocWordMass) {                                                   /* WRK:529-531 */
                    st->topic_doc_mass_cnt++;
                    const int lb = orc_lower_bound(topicDocWordMasses, sample, nonZeroTopics);     /* WRK:257-277 */
                    if (lb < 0) return 1;
                    newTopic = localTopicIndex[lb];
                } else {                                                                           /* WRK:533-535 */
                    st->word_ftree_mass_cnt++;
                    newTopic = orc_ftree_sample(currentTree, K, nextUniform2);                     /* FT:111-136 */
                    if (newTopic == -2) return 1;
                }
            }
            if (newTopic == -1) newTopic = K - 1;                                                  /* WRK:549-552 */
            o->z[m][base + position] = newTopic;                                                   /* WRK:557 */
            localTopicCounts[(size_t)m * K + newTopic]++;                                          /* WRK:560; the list never grows (WRK:563-584) */
            st->tokens++;
            if (newTopic != oldTopic) {                                                            /* WRK:587-589 */
                st->changed++;
                mxr_delta dl = { oldTopic, newTopic, type, m,
                                 (int64_t)(((uint64_t)doc_global << 34) | ((uint64_t)m << 31) | ((uint64_t)position << 11) | (uint64_t)newTopic) };
                dv_push(dv, dl);
            }
        }
    }
    return 0;
}

/* UPD:181-272 as one updater draining one queue; the two FTree.update calls (UPD:244-260) are the rebuild at the next sweep start */
static void apply_deltas(orc_model* o, const mxr_dvec* dv, orc_stats* st, int32_t* delta_nwk, int32_t* delta_nk, int apply)
{
    const int K = o->K;
    for (size_t i = 0; i < dv->n; i++) {
        const mxr_delta* dl = &dv->v[i];
        const size_t row = (size_t)(o->rowbase[dl->mod] + dl->type) * K;
        if (dl->oldT != -1) {                                                                      /* UPD:199-216 */
            if (apply) { o->nwk[row + dl->oldT]--; o->nk[(size_t)dl->mod * K + dl->oldT]--; }
            if (delta_nwk) delta_nwk[row + dl->oldT]--;
            if (delta_nk) delta_nk[(size_t)dl->mod * K + dl->oldT]--;
        }
        if (apply) { o->nwk[row + dl->newT]++; o->nk[(size_t)dl->mod * K + dl->newT]++; }          /* UPD:207,218 */
        if (delta_nwk) delta_nwk[row + dl->newT]++;
        if (delta_nk) delta_nk[(size_t)dl->mod * K + dl->newT]++;
        if (o->inactive[dl->newT] && dl->key < st->activation_key) {                               /* UPD:263-270: the first delta in (entity, view, position) order */
            st->activated_topic = dl->newT; st->activated_modality = dl->mod; st->activation_key = dl->key;
        }
    }
    if (apply && st->activated_topic >= 0) {
        o->inactive[st->activated_topic] = 0;
        o->alpha[(size_t)st->activated_modality * (K + 1) + st->activated_topic] = o->alpha[(size_t)st->activated_modality * (K + 1) + K];
    }
}

/* One deferred sweep.  doc_list == NULL: every entity in order; else the listed entities (local indices, list order): one segment.
 * flags: MXR_REUSE_TREES (no rebuild), MXR_NO_APPLY (deltas reported, model untouched), MXR_FROZEN (no deltas at all; the document term
 * without the mix: the inferencer's worker has lambda = 0, INF:251-252; trees as they stand). */
int mxr_sweep(orc_model* o, int use_mix, const double* mix, double oml, uint32_t sweep_idx, uint64_t seed, int64_t doc_id_base,
              const double* p_in, uint32_t flags, orc_stats* st, int32_t* delta_nwk, int32_t* delta_nk, double* const* tok_dbg,
              int n_trace, const int64_t* trace_doc, const int32_t* trace_view, const int32_t* trace_pos, double* trace_out,
              const int64_t* doc_list, int64_t n_list)
{
    const int K = o->K, M = o->M;
    orc_stats local; memset(&local, 0, sizeof local);
    local.activated_topic = -1; local.activated_modality = -1; local.activation_key = INT64_MAX;
    if (!(flags & (MXR_REUSE_TREES | MXR_FROZEN))) mxr_build_trees(o, use_mix, mix, oml);
    const int mix_docs = use_mix && !(flags & MXR_FROZEN);

    int first_inactive = -1;                                                                       /* inActiveTopicIndex.first() WRK:525 */
    for (int k = 0; k < K; k++) if (o->inactive[k]) { first_inactive = k; break; }
    double* p_own = NULL;
    const double* p = p_in;
    if (!p) {
        p_own = (double*)malloc((size_t)(o->D > 0 ? o->D : 1) * M * M * sizeof(double));
        orc_draw_p_philox(o, seed, sweep_idx, doc_id_base, p_own);
        p = p_own;
    }
    if (delta_nwk) memset(delta_nwk, 0, (size_t)o->rowbase[M] * K * sizeof(int32_t));
    if (delta_nk) memset(delta_nk, 0, (size_t)M * K * sizeof(int32_t));
    int32_t* localTopicCounts = (int32_t*)malloc((size_t)M * K * sizeof(int32_t));
    int32_t* localTopicIndex = (int32_t*)malloc((size_t)(K + 1) * sizeof(int32_t));
    double* topicDocWordMasses = (double*)malloc((size_t)(K + 1) * sizeof(double));
    double* totalMassOtherModalities = (double*)malloc((size_t)K * sizeof(double));
    double* terms = (double*)malloc((size_t)(K + 1) * sizeof(double));
    mxr_dvec dv = { NULL, 0, 0 };

    const int64_t n_visit = doc_list ? n_list : o->D;
    for (int64_t q = 0; q < n_visit; q++) {
        const int64_t d = doc_list ? doc_list[q] : q;
        if (d < 0 || d >= o->D) continue;
        memset(localTopicIndex, 0, (size_t)(K + 1) * sizeof(int32_t));
        topicDocWordMasses[0] = 0;
        if (sample_one_doc(o, mix_docs, mix, oml, d, doc_id_base + d, sweep_idx, seed, p + (size_t)d * M * M, first_inactive, &local, &dv, tok_dbg,
                           n_trace, trace_doc, trace_view, trace_pos, trace_out, (flags & MXR_TRACE_PRODUCT) != 0, terms,
                           localTopicCounts, localTopicIndex, topicDocWordMasses, totalMassOtherModalities)) local.aborted_docs++;
    }
    if (flags & MXR_FROZEN) { dv.n = 0; local.changed = 0; }                                       /* nut == 0: no FastQDelta is queued */
    apply_deltas(o, &dv, &local, delta_nwk, delta_nk, !(flags & MXR_NO_APPLY));
    free(dv.v); free(localTopicCounts); free(localTopicIndex); free(topicDocWordMasses); free(totalMassOtherModalities); free(terms); free(p_own);
    if (st) *st = local;
    return 0;
}
