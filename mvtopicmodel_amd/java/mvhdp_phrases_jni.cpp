// mvhdp_phrases_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativePhrases and mvhdp_topic_phrases of libmvhdp.so (include/mvhdp.h):
// findTopicPhrases (PTM:1921-1976) on the device, the call that replaces PTM:1555-1586 of saveTopicsandExperiment.  A source of its own
// beside mvhdp_jni.cpp and mvhdp_sim_jni.cpp, built INTO THE SAME libmvhdp_jni.so (add this file to that command line); everything it
// defines outside the entry lives in namespace mvhdp_phrases_jni, so the three sources also compile as one translation unit.
//
// The discipline is mvhdp_jni.cpp's: arrays cross with Get<Type>ArrayElements / Release<Type>ArrayElements, never through a critical
// region (the call blocks); no Get while an exception is pending; every array length is checked, as a jlong, before the library sees a
// pointer; a negative status becomes a RuntimeException carrying mvhdp_last_error().
//
// The jlong the entry takes is NativeSampler's handle: a pointer to the Shard of mvhdp_jni.cpp, whose leading members ShardHead restates
// (the library handle and the shape the checks need).  The sampler must stay open for the duration of the call.
#include <jni.h>

#include <cstdio>

#include "mvhdp.h"

namespace mvhdp_phrases_jni {

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
static_assert(sizeof(jint) == sizeof(int32_t) && sizeof(jlong) == sizeof(int64_t), "JNI primitive sizes");

}  // namespace mvhdp_phrases_jni

namespace pj = mvhdp_phrases_jni;

extern "C" {

// mvhdp_topic_phrases.  topicOff: long[K + 1] or null; distinct, occurrences: long[K] or null.  wordOff, counts: both null, or
// wordOff.length == counts.length + 1, and counts.length is the phrase capacity; words: null or an array whose length is the word capacity.
// All three null: the sizes only.  sizesOut: long[2] = phrases kept, their words.  statsOut: long[5] = runs, occurrences, distinct, kept,
// hash_collisions, or null.  Returns the number of phrases kept; when a size exceeds its capacity the arrays are untouched and no
// exception is raised (the caller repeats the call with arrays of the sizes in sizesOut).
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativePhrases_nTopicPhrases(JNIEnv* env, jclass, jlong handle, jint maxPerTopic, jint hashBits, jlongArray topicOff,
        jlongArray wordOff, jintArray words, jintArray counts, jlongArray distinct, jlongArray occurrences, jlongArray sizesOut, jlongArray statsOut)
{
    pj::ShardHead* s = pj::shard_of(env, handle);
    if (!s) return 0;
    if (topicOff && pj::bad_len(env, topicOff, (jlong)s->K + 1, "topicPhrases topicOff")) return 0;
    if (distinct && pj::bad_len(env, distinct, s->K, "topicPhrases distinct")) return 0;
    if (occurrences && pj::bad_len(env, occurrences, s->K, "topicPhrases occurrences")) return 0;
    jlong capPhrases = 0, capWords = 0;
    if (wordOff || counts) {
        if (!counts) { pj::throw_arg(env, "topicPhrases: wordOff and counts are given together or not at all"); return 0; }
        capPhrases = env->GetArrayLength(counts);
        if (pj::bad_len(env, wordOff, capPhrases + 1, "topicPhrases wordOff")) return 0;
    }
    if (words) {
        if (!counts) { pj::throw_arg(env, "topicPhrases: words without wordOff and counts"); return 0; }
        capWords = env->GetArrayLength(words);
    }
    if (pj::bad_len(env, sizesOut, 2, "topicPhrases sizesOut")) return 0;
    if (statsOut && pj::bad_len(env, statsOut, 5, "topicPhrases statsOut")) return 0;
    pj::Longs to(env, topicOff, 0), wo(env, wordOff, 0);
    pj::Ints w(env, words, 0), c(env, counts, 0);
    pj::Longs di(env, distinct, 0), oc(env, occurrences, 0), sz(env, sizesOut, 0), st(env, statsOut, 0);
    if (to.failed() || wo.failed() || w.failed() || c.failed() || di.failed() || oc.failed() || sz.failed() || st.failed()) return 0;
    mvhdp_phrase_args a{};
    a.max_per_topic = maxPerTopic; a.hash_bits = hashBits;
    mvhdp_phrase_stats ps{};
    int64_t nPhrases = 0, nWords = 0;
    const int rc = mvhdp_topic_phrases(s->h, &a, capPhrases, capWords, to.p, wo.p, w.p, c.p, di.p, oc.p, &nPhrases, &nWords, &ps);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && (nPhrases > capPhrases || nWords > capWords))) { pj::throw_rt(env, s->h, rc, "mvhdp_topic_phrases"); return 0; }
    sz.p[0] = nPhrases; sz.p[1] = nWords;
    if (st.p && rc == MVHDP_OK) { st.p[0] = ps.runs; st.p[1] = ps.occurrences; st.p[2] = ps.distinct; st.p[3] = ps.kept; st.p[4] = ps.hash_collisions; }
    return nPhrases;
}

}  // extern "C"
