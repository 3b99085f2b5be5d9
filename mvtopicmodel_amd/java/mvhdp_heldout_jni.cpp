// mvhdp_heldout_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativeHeldout and mvhdp_heldout_left_to_right of libmvhdp.so
// (include/mvhdp.h): the left-to-right held-out likelihood on the device, the call that replaces
// getMALLETProbEstimator().evaluateLeftToRight(testing, particles, resample, null) (PTM:3470-3478).  A source of its own beside
// mvhdp_jni.cpp, mvhdp_sim_jni.cpp and mvhdp_phrases_jni.cpp, built INTO THE SAME libmvhdp_jni.so (add this file to that command line);
// everything it defines outside the entry lives in namespace mvhdp_heldout_jni, so the four sources also compile as one translation unit.
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

namespace mvhdp_heldout_jni {

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

}  // namespace mvhdp_heldout_jni

namespace hj = mvhdp_heldout_jni;

extern "C" {

// mvhdp_heldout_left_to_right.  docOff: long[D + 1], D >= 0, docOff[0] == 0; tokens: int[docOff[D]].  alpha: double[K] (then alphaSum is
// used) or null.  docLl: double[D] or null; positionSum: double[docOff[D]] or null; docTokens: long[D] or null; statsOut: long[3] = tokens,
// oov, visits, or null.  Returns the total log-likelihood.
JNIEXPORT jdouble JNICALL Java_org_madgik_MVTopicModel_NativeHeldout_nLeftToRight(JNIEnv* env, jclass, jlong handle, jint m, jint particles, jint resample, jlong seed,
        jlong docBase, jdoubleArray alpha, jdouble alphaSum, jlongArray docOff, jintArray tokens, jdoubleArray docLl, jdoubleArray positionSum, jlongArray docTokens,
        jlongArray statsOut)
{
    hj::ShardHead* s = hj::shard_of(env, handle);
    if (!s) return 0;
    if (!docOff || env->GetArrayLength(docOff) < 1) { hj::throw_arg(env, "heldout docOff: at least one entry expected"); return 0; }
    const jlong D = (jlong)env->GetArrayLength(docOff) - 1;
    jlong N = 0;
    env->GetLongArrayRegion(docOff, (jsize)D, 1, &N);          // the last entry: what the token arrays are measured against
    if (env->ExceptionCheck()) return 0;
    if (N < 0) { hj::throw_arg(env, "heldout docOff: negative token count"); return 0; }
    if (hj::bad_len(env, tokens, N, "heldout tokens")) return 0;
    if (alpha && hj::bad_len(env, alpha, s->K, "heldout alpha")) return 0;
    if (docLl && hj::bad_len(env, docLl, D, "heldout docLl")) return 0;
    if (positionSum && hj::bad_len(env, positionSum, N, "heldout positionSum")) return 0;
    if (docTokens && hj::bad_len(env, docTokens, D, "heldout docTokens")) return 0;
    if (statsOut && hj::bad_len(env, statsOut, 3, "heldout statsOut")) return 0;
    hj::Longs off(env, docOff, JNI_ABORT);
    hj::Ints tok(env, tokens, JNI_ABORT);
    hj::Doubles al(env, alpha, JNI_ABORT), ll(env, docLl, 0), ps(env, positionSum, 0);
    hj::Longs dt(env, docTokens, 0), st(env, statsOut, 0);
    if (off.failed() || tok.failed() || al.failed() || ll.failed() || ps.failed() || dt.failed() || st.failed()) return 0;
    mvhdp_heldout_args a{};
    a.m = m; a.particles = particles; a.resample = resample; a.seed = (uint64_t)seed; a.doc_base = docBase;
    a.alpha = al.p; a.alpha_sum = alphaSum;
    mvhdp_heldout_stats hs{};
    const int rc = mvhdp_heldout_left_to_right(s->h, &a, D, off.p, tok.p, ll.p, ps.p, dt.p, &hs);
    if (rc != MVHDP_OK) { hj::throw_rt(env, s->h, rc, "mvhdp_heldout_left_to_right"); return 0; }
    if (st.p) { st.p[0] = hs.tokens; st.p[1] = hs.oov; st.p[2] = hs.visits; }
    return hs.log_likelihood;
}

}  // extern "C"
