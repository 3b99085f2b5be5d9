// mvhdp_sim_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativeSimilarity and the three post-training entry points of
// libmvhdp.so (include/mvhdp.h: mvhdp_similar_pairs, mvhdp_doc_topics_top, mvhdp_entity_topic_distributions).  A source of its own beside
// mvhdp_jni.cpp, built INTO THE SAME libmvhdp_jni.so (add this file to that command line); everything it defines outside the entries
// lives in namespace mvhdp_sim_jni, so the two sources also compile as one translation unit.
//
// The discipline is mvhdp_jni.cpp's: arrays cross with Get<Type>ArrayElements / Release<Type>ArrayElements, never through a critical
// region (every mvhdp_* call here blocks); no Get while an exception is pending; every array length is checked, as a jlong product,
// before the library sees a pointer; a negative status becomes a RuntimeException carrying mvhdp_last_error().
//
// The jlong these entries take is NativeSampler's handle: a pointer to the Shard of mvhdp_jni.cpp, whose leading members ShardHead
// restates (the library handle and the shape the checks need).  The sampler must stay open for the duration of the call.
#include <jni.h>

#include <cstdio>
#include <vector>

#include "mvhdp.h"

namespace mvhdp_sim_jni {

struct ShardHead {                   // = the leading members of mvhdp_jni.cpp's Shard, in its order
    mvhdp_handle h;
    int K, M;
    int V[MVHDP_MAX_MODALITIES];
    jlong D;
};

void throw_msg(JNIEnv* env, const char* cls, const char* msg)
{
    jclass c = env->FindClass(cls);
    if (c) env->ThrowNew(c, msg);
}

void throw_rt(JNIEnv* env, mvhdp_handle h, int rc, const char* what)
{
    char msg[640];
    snprintf(msg, sizeof msg, "%s failed (%d): %s", what, rc, mvhdp_last_error(h));
    throw_msg(env, "java/lang/RuntimeException", msg);
}

void throw_arg(JNIEnv* env, const char* msg) { throw_msg(env, "java/lang/IllegalArgumentException", msg); }

bool bad_len(JNIEnv* env, jarray a, jlong want, const char* what)
{
    if (a && env->GetArrayLength(a) == want) return false;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: array of length %lld expected, got %lld", what, (long long)want, a ? (long long)env->GetArrayLength(a) : -1LL);
    throw_arg(env, msg);
    return true;
}

ShardHead* shard_of(JNIEnv* env, jlong handle)
{
    ShardHead* s = reinterpret_cast<ShardHead*>(handle);
    if (!s || !s->h) { throw_msg(env, "java/lang/IllegalStateException", "NativeSampler is closed"); return nullptr; }
    return s;
}

// RAII over Get/Release<Type>ArrayElements (mode 0: copy back and free; JNI_ABORT: input only).  Once one Get has failed
// (OutOfMemoryError pending) the next ones take nothing and report failed() as well.
struct Ints {
    JNIEnv* env; jintArray a; jint* p; jint mode;
    Ints(JNIEnv* e, jintArray arr, jint m) : env(e), a(arr), p(arr && !e->ExceptionCheck() ? e->GetIntArrayElements(arr, nullptr) : nullptr), mode(m) {}
    ~Ints() { if (a && p) env->ReleaseIntArrayElements(a, p, mode); }
    bool failed() const { return a && !p; }
};
struct Longs {
    JNIEnv* env; jlongArray a; jlong* p; jint mode;
    Longs(JNIEnv* e, jlongArray arr, jint m) : env(e), a(arr), p(arr && !e->ExceptionCheck() ? e->GetLongArrayElements(arr, nullptr) : nullptr), mode(m) {}
    ~Longs() { if (a && p) env->ReleaseLongArrayElements(a, p, mode); }
    bool failed() const { return a && !p; }
};
struct Doubles {
    JNIEnv* env; jdoubleArray a; jdouble* p; jint mode;
    Doubles(JNIEnv* e, jdoubleArray arr, jint m) : env(e), a(arr), p(arr && !e->ExceptionCheck() ? e->GetDoubleArrayElements(arr, nullptr) : nullptr), mode(m) {}
    ~Doubles() { if (a && p) env->ReleaseDoubleArrayElements(a, p, mode); }
    bool failed() const { return a && !p; }
};

static_assert(sizeof(jint) == sizeof(int32_t) && sizeof(jlong) == sizeof(int64_t) && sizeof(jdouble) == sizeof(double), "JNI primitive sizes");

}  // namespace mvhdp_sim_jni

namespace sj = mvhdp_sim_jni;     // (a using-directive would collide with mvhdp_jni.cpp's helpers of the same names in a joint translation unit)

extern "C" {

// All pairs i < j of the n rows of xFlat [n * dim] with sim > threshold.  i, j, sim: all null (count only) or three arrays of one length,
// the capacity.  Returns the number of pairs; when that exceeds the capacity the arrays are untouched and no exception is raised (the
// caller repeats the call with arrays of that length).  statsOut: long[5] = pairs_screened, candidates, emitted, stripes, regrown, or
// null; marginOut: double[1] or null.
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nSimilarPairs(JNIEnv* env, jclass, jlong handle, jint metric, jint n, jint dim, jdoubleArray xFlat,
        jdouble minWeight, jdouble threshold, jint stripeRows, jlong candidateCapacity, jintArray i, jintArray j, jdoubleArray sim, jlongArray statsOut, jdoubleArray marginOut)
{
    sj::ShardHead* s = sj::shard_of(env, handle);
    if (!s) return 0;
    if (n < 0 || dim < 1) { sj::throw_arg(env, "similarPairs: n >= 0 and dim >= 1 expected"); return 0; }
    if (sj::bad_len(env, xFlat, (jlong)n * (jlong)dim, "similarPairs xFlat")) return 0;
    jlong cap = 0;
    if (i || j || sim) {
        if (!i) { sj::throw_arg(env, "similarPairs: i, j and sim are given together or not at all"); return 0; }
        cap = env->GetArrayLength(i);
        if (sj::bad_len(env, j, cap, "similarPairs j") || sj::bad_len(env, sim, cap, "similarPairs sim")) return 0;
    }
    if (statsOut && sj::bad_len(env, statsOut, 5, "similarPairs statsOut")) return 0;
    if (marginOut && sj::bad_len(env, marginOut, 1, "similarPairs marginOut")) return 0;
    sj::Doubles x(env, xFlat, JNI_ABORT);
    sj::Ints oi(env, i, 0), oj(env, j, 0);
    sj::Doubles os(env, sim, 0);
    sj::Longs st(env, statsOut, 0);
    sj::Doubles mg(env, marginOut, 0);
    if (x.failed() || oi.failed() || oj.failed() || os.failed() || st.failed() || mg.failed()) return 0;
    mvhdp_sim_args a{};
    a.metric = metric; a.n = n; a.dim = dim; a.x = x.p; a.min_weight = minWeight; a.threshold = threshold;
    a.stripe_rows = stripeRows; a.candidate_capacity = candidateCapacity;
    mvhdp_sim_stats ss{};
    int64_t count = 0;
    const int rc = mvhdp_similar_pairs(s->h, &a, cap, oi.p, oj.p, os.p, &count, &ss);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && count > cap)) { sj::throw_rt(env, s->h, rc, "mvhdp_similar_pairs"); return 0; }
    if (st.p) { st.p[0] = ss.pairs_screened; st.p[1] = ss.candidates; st.p[2] = ss.emitted; st.p[3] = ss.stripes; st.p[4] = ss.regrown; }
    if (mg.p) mg.p[0] = ss.margin;
    return count;
}

// PTM:2890-2926 for entities [d0, d1).  rowOff: long[d1 - d0 + 1] or null; topics, weights: both null (count only) or two arrays of one
// length, the capacity.  Returns the number of entries; beyond the capacity as nSimilarPairs.
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nDocTopicsTop(JNIEnv* env, jclass, jlong handle, jdoubleArray viewWeights, jlong d0, jlong d1,
        jdouble threshold, jint max, jlongArray rowOff, jintArray topics, jdoubleArray weights)
{
    sj::ShardHead* s = sj::shard_of(env, handle);
    if (!s) return 0;
    if (sj::bad_len(env, viewWeights, s->M, "docTopicsTop viewWeights")) return 0;
    if (d0 < 0 || d1 < d0 || d1 > s->D) { sj::throw_arg(env, "docTopicsTop: 0 <= d0 <= d1 <= numEntities expected"); return 0; }
    if (rowOff && sj::bad_len(env, rowOff, d1 - d0 + 1, "docTopicsTop rowOff")) return 0;
    jlong cap = 0;
    if (topics || weights) {
        if (!topics) { sj::throw_arg(env, "docTopicsTop: topics and weights are given together or not at all"); return 0; }
        cap = env->GetArrayLength(topics);
        if (sj::bad_len(env, weights, cap, "docTopicsTop weights")) return 0;
    }
    sj::Doubles w(env, viewWeights, JNI_ABORT);
    sj::Longs off(env, rowOff, 0);
    sj::Ints t(env, topics, 0);
    sj::Doubles wt(env, weights, 0);
    if (w.failed() || off.failed() || t.failed() || wt.failed()) return 0;
    int64_t count = 0;
    const int rc = mvhdp_doc_topics_top(s->h, w.p, d0, d1, threshold, max, cap, off.p, t.p, wt.p, &count);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && count > cap)) { sj::throw_rt(env, s->h, rc, "mvhdp_doc_topics_top"); return 0; }
    return count;
}

// FLOW:807-1083 as include/mvhdp.h defines it.  memberOff: long[nGroups + 1]; members: long[memberOff[nGroups]]; out: double[nGroups * K].
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_nEntityTopicDistributions(JNIEnv* env, jclass, jlong handle, jdoubleArray viewWeights, jdouble threshold,
        jint max, jint roundDigits, jlongArray memberOff, jlongArray members, jdoubleArray out)
{
    sj::ShardHead* s = sj::shard_of(env, handle);
    if (!s) return;
    if (sj::bad_len(env, viewWeights, s->M, "entityTopicDistributions viewWeights")) return;
    if (!memberOff || env->GetArrayLength(memberOff) < 1) { sj::throw_arg(env, "entityTopicDistributions: memberOff of length nGroups + 1 expected"); return; }
    const jlong nGroups = (jlong)env->GetArrayLength(memberOff) - 1;
    if (sj::bad_len(env, out, nGroups * (jlong)s->K, "entityTopicDistributions out")) return;
    if (!members) { sj::throw_arg(env, "entityTopicDistributions: members is null"); return; }
    const jlong nMembers = env->GetArrayLength(members);
    sj::Doubles w(env, viewWeights, JNI_ABORT);
    sj::Longs off(env, memberOff, JNI_ABORT), mem(env, members, JNI_ABORT);
    sj::Doubles o(env, out, 0);
    if (w.failed() || off.failed() || mem.failed() || o.failed()) return;
    if (off.p[0] != 0 || off.p[nGroups] != nMembers) { sj::throw_arg(env, "entityTopicDistributions: memberOff must run from 0 to members.length"); return; }
    for (jlong g = 0; g < nGroups; g++)
        if (off.p[g + 1] < off.p[g]) { sj::throw_arg(env, "entityTopicDistributions: memberOff decreases"); return; }
    const int rc = mvhdp_entity_topic_distributions(s->h, w.p, threshold, max, roundDigits, nGroups, off.p, mem.p, o.p);
    if (rc != MVHDP_OK) sj::throw_rt(env, s->h, rc, "mvhdp_entity_topic_distributions");
}

}  // extern "C"
