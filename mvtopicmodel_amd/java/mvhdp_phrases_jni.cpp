// mvhdp_phrases_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativePhrases and mvhdp_topic_phrases of libmvhdp.so (include/mvhdp.h):
// findTopicPhrases (PTM:1921-1976) on the device, the call that replaces PTM:1555-1586 of saveTopicsandExperiment.  A source of its own
// beside mvhdp_jni.cpp and mvhdp_sim_jni.cpp, built INTO THE SAME libmvhdp_jni.so (the command line at the head of mvhdp_jni.cpp names
// it); it defines nothing but its entry, so the shim sources also compile as one translation unit.
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
using mvhdp_jni::Ints; using mvhdp_jni::Longs;

extern "C" {

// mvhdp_topic_phrases.  topicOff: long[K + 1] or null; distinct, occurrences: long[K] or null.  wordOff, counts: both null, or
// wordOff.length == counts.length + 1, and counts.length is the phrase capacity; words: null or an array whose length is the word capacity.
// All three null: the sizes only.  sizesOut: long[2] = phrases kept, their words.  statsOut: long[5] = runs, occurrences, distinct, kept,
// hash_collisions, or null.  Returns the number of phrases kept; when a size exceeds its capacity the arrays are untouched and no
// exception is raised (the caller repeats the call with arrays of the sizes in sizesOut).
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativePhrases_nTopicPhrases(JNIEnv* env, jclass, jlong handle, jint maxPerTopic, jint hashBits, jlongArray topicOff,
        jlongArray wordOff, jintArray words, jintArray counts, jlongArray distinct, jlongArray occurrences, jlongArray sizesOut, jlongArray statsOut)
{
    ShardPin pin_(env, handle); Shard* s = pin_.s;
    if (!s) return 0;
    if (topicOff && bad_len(env, topicOff, (jlong)s->K + 1, "topicPhrases topicOff")) return 0;
    if (distinct && bad_len(env, distinct, s->K, "topicPhrases distinct")) return 0;
    if (occurrences && bad_len(env, occurrences, s->K, "topicPhrases occurrences")) return 0;
    jlong capPhrases = 0, capWords = 0;
    if (wordOff || counts) {
        if (!counts) { throw_arg(env, "topicPhrases: wordOff and counts are given together or not at all"); return 0; }
        capPhrases = env->GetArrayLength(counts);
        if (bad_len(env, wordOff, capPhrases + 1, "topicPhrases wordOff")) return 0;
    }
    if (words) {
        if (!counts) { throw_arg(env, "topicPhrases: words without wordOff and counts"); return 0; }
        capWords = env->GetArrayLength(words);
    }
    if (bad_len(env, sizesOut, 2, "topicPhrases sizesOut")) return 0;
    if (statsOut && bad_len(env, statsOut, 5, "topicPhrases statsOut")) return 0;
    Longs to(env, topicOff, 0), wo(env, wordOff, 0);
    Ints w(env, words, 0), c(env, counts, 0);
    Longs di(env, distinct, 0), oc(env, occurrences, 0), sz(env, sizesOut, 0), st(env, statsOut, 0);
    if (to.failed() || wo.failed() || w.failed() || c.failed() || di.failed() || oc.failed() || sz.failed() || st.failed()) return 0;
    mvhdp_phrase_args a{};
    a.max_per_topic = maxPerTopic; a.hash_bits = hashBits;
    mvhdp_phrase_stats ps{};
    int64_t nPhrases = 0, nWords = 0;
    const int rc = mvhdp_topic_phrases(s->h, &a, capPhrases, capWords, to.p, wo.p, w.p, c.p, di.p, oc.p, &nPhrases, &nWords, &ps);
    if (rc != MVHDP_OK && !(rc == MVHDP_ERR_INVALID_ARG && (nPhrases > capPhrases || nWords > capWords))) { throw_rt(env, s->h, rc, "mvhdp_topic_phrases"); return 0; }
    sz.p[0] = nPhrases; sz.p[1] = nWords;
    if (st.p && rc == MVHDP_OK) { st.p[0] = ps.runs; st.p[1] = ps.occurrences; st.p[2] = ps.distinct; st.p[3] = ps.kept; st.p[4] = ps.hash_collisions; }
    return nPhrases;
}

}  // extern "C"
