// mvhdp_heldout_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativeHeldout and mvhdp_heldout_left_to_right of libmvhdp.so
// (include/mvhdp.h): the left-to-right held-out likelihood on the device, the call that replaces
// getMALLETProbEstimator().evaluateLeftToRight(testing, particles, resample, null) (PTM:3470-3478).  A source of its own beside
// mvhdp_jni.cpp, mvhdp_sim_jni.cpp and mvhdp_phrases_jni.cpp, built INTO THE SAME libmvhdp_jni.so (the command line at the head of
// mvhdp_jni.cpp names it); it defines nothing but its entry, so the four sources also compile as one translation unit.
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

// mvhdp_heldout_left_to_right.  docOff: long[D + 1], D >= 0, docOff[0] == 0; tokens: int[docOff[D]].  alpha: double[K] (then alphaSum is
// used) or null.  docLl: double[D] or null; positionSum: double[docOff[D]] or null; docTokens: long[D] or null; statsOut: long[3] = tokens,
// oov, visits, or null.  Returns the total log-likelihood.
JNIEXPORT jdouble JNICALL Java_org_madgik_MVTopicModel_NativeHeldout_nLeftToRight(JNIEnv* env, jclass, jlong handle, jint m, jint particles, jint resample, jlong seed,
        jlong docBase, jdoubleArray alpha, jdouble alphaSum, jlongArray docOff, jintArray tokens, jdoubleArray docLl, jdoubleArray positionSum, jlongArray docTokens,
        jlongArray statsOut)
{
    ShardPin pin_(env, handle); Shard* s = pin_.s;
    if (!s) return 0;
    if (!docOff || env->GetArrayLength(docOff) < 1) { throw_arg(env, "heldout docOff: at least one entry expected"); return 0; }
    const jlong D = (jlong)env->GetArrayLength(docOff) - 1;
    jlong N = 0;
    env->GetLongArrayRegion(docOff, (jsize)D, 1, &N);          // the last entry: what the token arrays are measured against
    if (env->ExceptionCheck()) return 0;
    if (N < 0) { throw_arg(env, "heldout docOff: negative token count"); return 0; }
    if (bad_len(env, tokens, N, "heldout tokens")) return 0;
    if (alpha && bad_len(env, alpha, s->K, "heldout alpha")) return 0;
    if (docLl && bad_len(env, docLl, D, "heldout docLl")) return 0;
    if (positionSum && bad_len(env, positionSum, N, "heldout positionSum")) return 0;
    if (docTokens && bad_len(env, docTokens, D, "heldout docTokens")) return 0;
    if (statsOut && bad_len(env, statsOut, 3, "heldout statsOut")) return 0;
    Longs off(env, docOff, JNI_ABORT);
    Ints tok(env, tokens, JNI_ABORT);
    Doubles al(env, alpha, JNI_ABORT), ll(env, docLl, 0), ps(env, positionSum, 0);
    Longs dt(env, docTokens, 0), st(env, statsOut, 0);
    if (off.failed() || tok.failed() || al.failed() || ll.failed() || ps.failed() || dt.failed() || st.failed()) return 0;
    mvhdp_heldout_args a{};
    a.m = m; a.particles = particles; a.resample = resample; a.seed = (uint64_t)seed; a.doc_base = docBase;
    a.alpha = al.p; a.alpha_sum = alphaSum;
    mvhdp_heldout_stats hs{};
    const int rc = mvhdp_heldout_left_to_right(s->h, &a, D, off.p, tok.p, ll.p, ps.p, dt.p, &hs);
    if (rc != MVHDP_OK) { throw_rt(env, s->h, rc, "mvhdp_heldout_left_to_right"); return 0; }
    if (st.p) { st.p[0] = hs.tokens; st.p[1] = hs.oov; st.p[2] = hs.visits; }
    return hs.log_likelihood;
}

}  // extern "C"
