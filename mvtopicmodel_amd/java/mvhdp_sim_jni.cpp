// mvhdp_sim_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativeSimilarity and the three post-training entry points of
// libmvhdp.so (include/mvhdp.h: mvhdp_similar_pairs, mvhdp_doc_topics_top, mvhdp_entity_topic_distributions).  A source of its own beside
// mvhdp_jni.cpp, built INTO THE SAME libmvhdp_jni.so (the command line at the head of mvhdp_jni.cpp names it); it defines nothing but its
// entries, so the shim sources also compile as one translation unit.
// What it shares with the other shim sources is mvhdp_jni_common.h; the discipline is mvhdp_jni.cpp's: arrays cross with
// Get<Type>ArrayElements / Release<Type>ArrayElements, never through a critical region (every mvhdp_* call here blocks); no Get while an
// exception is pending; every array length is checked, as a jlong, before the library sees a pointer; a negative status becomes a
// RuntimeException carrying mvhdp_last_error().
//
// The jlong an entry takes is NativeSampler's handle.  It is looked up in the shim's registry and PINNED for the call exactly as the
// NativeSampler entries do it (ShardPin): a handle that is closed, or was never issued, is refused with IllegalStateException instead of
// dereferenced, and a close() on another thread waits for the call to return.
#include "mvhdp_jni_common.h"

using mvhdp_jni::ShardPin; using mvhdp_jni::Shard; using mvhdp_jni::throw_arg; using mvhdp_jni::throw_rt; using mvhdp_jni::bad_len;
using mvhdp_jni::Ints; using mvhdp_jni::Longs; using mvhdp_jni::Doubles;

extern "C" {

// All pairs i < j of the n rows of xFlat [n * dim] with sim > threshold.  i, j, sim: all null (count only) or three arrays of one length,
// the capacity.  Returns the number of pairs; when that exceeds the capacity the arrays are untouched and no exception is raised (the
// caller repeats the call with arrays of that length).  statsOut: long[5] = pairs_screened, candidates, emitted, stripes, regrown, or
// null; marginOut: double[1] or null.
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nSimilarPairs(JNIEnv* env, jclass, jlong handle, jint metric, jint n, jint dim, jdoubleArray xFlat,
        jdouble minWeight, jdouble threshold, jint stripeRows, jlong candidateCapacity, jintArray i, jintArray j, jdoubleArray sim, jlongArray statsOut, jdoubleArray marginOut)
{
    ShardPin pin_(env, handle); Shard* s = pin_.s;
    if (!s) return 0;
    if (n < 0 || dim < 1) { throw_arg(env, "similarPairs: n >= 0 and dim >= 1 expected"); return 0; }
    if (bad_len(env, xFlat, (jlong)n * (jlong)dim, "similarPairs xFlat")) return 0;
    jlong cap = 0;
    if (i || j || sim) {
        if (!i) { throw_arg(env, "similarPairs: i, j and sim are given together or not at all"); return 0; }
        cap = env->GetArrayLength(i);
        if (bad_len(env, j, cap, "similarPairs j") || bad_len(env, sim, cap, "similarPairs sim")) return 0;
    }
    if (statsOut && bad_len(env, statsOut, 5, "similarPairs statsOut")) return 0;
    if (marginOut && bad_len(env, marginOut, 1, "similarPairs marginOut")) return 0;
    Doubles x(env, xFlat, JNI_ABORT);
    Ints oi(env, i, 0), oj(env, j, 0);
    Doubles os(env, sim, 0);
    Longs st(env, statsOut, 0);
    Doubles mg(env, marginOut, 0);
    if (x.failed() || oi.failed() || oj.failed() || os.failed() || st.failed() || mg.failed()) return 0;
    mvhdp_sim_args a{};
    a.metric = metric; a.n = n; a.dim = dim; a.x = x.p; a.min_weight = minWeight; a.threshold = threshold;
    a.stripe_rows = stripeRows; a.candidate_capacity = candidateCapacity;
    mvhdp_sim_stats ss{};
    int64_t count = 0;
    const int rc = mvhdp_similar_pairs(s->h, &a, cap, oi.p, oj.p, os.p, &count, &ss);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && count > cap)) { throw_rt(env, s->h, rc, "mvhdp_similar_pairs"); return 0; }
    if (st.p) { st.p[0] = ss.pairs_screened; st.p[1] = ss.candidates; st.p[2] = ss.emitted; st.p[3] = ss.stripes; st.p[4] = ss.regrown; }
    if (mg.p) mg.p[0] = ss.margin;
    return count;
}

// PTM:2890-2926 for entities [d0, d1).  rowOff: long[d1 - d0 + 1] or null; topics, weights: both null (count only) or two arrays of one
// length, the capacity.  Returns the number of entries; beyond the capacity as nSimilarPairs.
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nDocTopicsTop(JNIEnv* env, jclass, jlong handle, jdoubleArray viewWeights, jlong d0, jlong d1,
        jdouble threshold, jint max, jlongArray rowOff, jintArray topics, jdoubleArray weights)
{
    ShardPin pin_(env, handle); Shard* s = pin_.s;
    if (!s) return 0;
    if (bad_len(env, viewWeights, s->M, "docTopicsTop viewWeights")) return 0;
    if (d0 < 0 || d1 < d0 || d1 > s->D) { throw_arg(env, "docTopicsTop: 0 <= d0 <= d1 <= numEntities expected"); return 0; }
    if (rowOff && bad_len(env, rowOff, d1 - d0 + 1, "docTopicsTop rowOff")) return 0;
    jlong cap = 0;
    if (topics || weights) {
        if (!topics) { throw_arg(env, "docTopicsTop: topics and weights are given together or not at all"); return 0; }
        cap = env->GetArrayLength(topics);
        if (bad_len(env, weights, cap, "docTopicsTop weights")) return 0;
    }
    Doubles w(env, viewWeights, JNI_ABORT);
    Longs off(env, rowOff, 0);
    Ints t(env, topics, 0);
    Doubles wt(env, weights, 0);
    if (w.failed() || off.failed() || t.failed() || wt.failed()) return 0;
    int64_t count = 0;
    const int rc = mvhdp_doc_topics_top(s->h, w.p, d0, d1, threshold, max, cap, off.p, t.p, wt.p, &count);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && count > cap)) { throw_rt(env, s->h, rc, "mvhdp_doc_topics_top"); return 0; }
    return count;
}

// FLOW:807-1083 as include/mvhdp.h defines it.  memberOff: long[nGroups + 1]; members: long[memberOff[nGroups]]; out: double[nGroups * K].
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nEntityTopicDistributions(JNIEnv* env, jclass, jlong handle, jdoubleArray viewWeights, jdouble threshold,
        jint max, jint roundDigits, jlongArray memberOff, jlongArray members, jdoubleArray out)
{
    ShardPin pin_(env, handle); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, viewWeights, s->M, "entityTopicDistributions viewWeights")) return;
    if (!memberOff || env->GetArrayLength(memberOff) < 1) { throw_arg(env, "entityTopicDistributions: memberOff of length nGroups + 1 expected"); return; }
    const jlong nGroups = (jlong)env->GetArrayLength(memberOff) - 1;
    if (bad_len(env, out, nGroups * (jlong)s->K, "entityTopicDistributions out")) return;
    if (!members) { throw_arg(env, "entityTopicDistributions: members is null"); return; }
    const jlong nMembers = env->GetArrayLength(members);
    Doubles w(env, viewWeights, JNI_ABORT);
    Longs off(env, memberOff, JNI_ABORT), mem(env, members, JNI_ABORT);
    Doubles o(env, out, 0);
    if (w.failed() || off.failed() || mem.failed() || o.failed()) return;
    if (off.p[0] != 0 || off.p[nGroups] != nMembers) { throw_arg(env, "entityTopicDistributions: memberOff must run from 0 to members.length"); return; }
    for (jlong g = 0; g < nGroups; g++)
        if (off.p[g + 1] < off.p[g]) { throw_arg(env, "entityTopicDistributions: memberOff decreases"); return; }
    const int rc = mvhdp_entity_topic_distributions(s->h, w.p, threshold, max, roundDigits, nGroups, off.p, mem.p, o.p);
    if (rc != MVHDP_OK) throw_rt(env, s->h, rc, "mvhdp_entity_topic_distributions");
}

}  // extern "C"
