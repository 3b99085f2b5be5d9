// mvhdp_jni_common.h — what the four shim sources of libmvhdp_jni.so share (mvhdp_jni.cpp, mvhdp_sim_jni.cpp, mvhdp_phrases_jni.cpp,
// mvhdp_heldout_jni.cpp): what a jlong handle points to, the registry of the handles Java holds, the exceptions, the array wrappers.
// A new shim source includes this file and defines its Java_* entries; it restates nothing.
//
// The registry is ONE object per libmvhdp_jni.so however the sources are built -- the four on one command line, or one translation unit
// that includes all four: its variables are C++17 inline variables of a named namespace, never static and never in an anonymous
// namespace (a registry per source would have every entry outside mvhdp_jni.cpp refuse every handle nCreate made).  The namespace is
// hidden: nothing of it is exported beside the Java_* entries.
#ifndef MVHDP_JNI_COMMON_H
#define MVHDP_JNI_COMMON_H
#include <jni.h>

#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <set>
#include <vector>

#include "mvhdp.h"

namespace mvhdp_jni __attribute__((visibility("hidden"))) {

struct Shard {                       // what the jlong handle points to: the library handle plus the shape for the checks
    mvhdp_handle h = nullptr;
    int K = 0, M = 0;
    int V[MVHDP_MAX_MODALITIES] = {};
    jlong D = -1;
    jlong N[MVHDP_MAX_MODALITIES] = {};
    jlong embR = 0;                  // rows of the embedding matrix (V_0, + K with topics); 0: none (nEmbInit .. nEmbRelease)
    int embC = 0, embK = 0;          //   its columns, its topic rows
    int pins = 0;                    // JNI calls currently inside the library on this handle (guarded by g_reg_mutex)
};

struct Group {                        // an mvhdp_group, how many members it has in this process, and the model's shape for the checks
    mvhdp_group g = nullptr;
    int members = 0;
    int K = 0, M = 0;                 // of the member Shards (validate_members: every member holds the same shape)
    std::vector<Shard*> shards;       // the members, PINNED from nGroupCreate to nGroupDestroy: nDestroy of a member (a finalizer, another thread)
                                      // waits for its pins, so a member cannot be destroyed under a group that still names it
    int pins = 0;
};

// Every Shard (and group) the shim has handed to Java is listed here; a jlong that is not listed -- closed already, e.g. by a
// finalizer racing an explicit close(), or never issued -- is refused instead of dereferenced.  A call that found its object PINS it
// for its duration: close() takes the object out of the registry at once (no new call can find it) and then waits until the calls
// already inside the library have returned before it frees anything -- a close() racing a sweep (or a similarity or held-out call, the
// longest there are) on another thread cannot pull the handle from under it.
inline std::mutex g_reg_mutex;
inline std::condition_variable g_reg_cv;
inline std::set<void*> g_shards, g_groups;

inline void throw_msg(JNIEnv* env, const char* cls, const char* msg)
{
    jclass c = env->FindClass(cls);
    if (c) env->ThrowNew(c, msg);
}

inline void throw_arg(JNIEnv* env, const char* msg) { throw_msg(env, "java/lang/IllegalArgumentException", msg); }

inline void throw_rt(JNIEnv* env, mvhdp_handle h, int rc, const char* what)
{
    char msg[640];
    snprintf(msg, sizeof msg, "%s failed (%d): %s", what, rc, mvhdp_last_error(h));
    throw_msg(env, "java/lang/RuntimeException", msg);
}

inline bool bad_len(JNIEnv* env, jarray a, jlong want, const char* what)
{
    if (a && env->GetArrayLength(a) == want) return false;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: array of length %lld expected, got %lld", what, (long long)want, a ? (long long)env->GetArrayLength(a) : -1LL);
    throw_arg(env, msg);
    return true;
}

// a pin that outlives the call that took it (a group's on its members); nullptr: the jlong is not registered
template <class T>
T* pin(std::set<void*>& reg, jlong p)
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    if (!reg.count(reinterpret_cast<void*>(p))) return nullptr;
    T* s = reinterpret_cast<T*>(p);
    s->pins++;
    return s;
}

template <class T>
void unpin(T* s)
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    if (--s->pins == 0) g_reg_cv.notify_all();
}

// The line that opens almost every entry: the object behind the jlong, pinned until the entry returns -- or, for a jlong that is not
// registered, s == nullptr and an IllegalStateException pending (the entry returns at once).
template <class T>
struct Pin {
    T* const s;
    Pin(JNIEnv* env, std::set<void*>& reg, jlong p, const char* closed) : s(pin<T>(reg, p))
    {
        if (!s) throw_msg(env, "java/lang/IllegalStateException", closed);
    }
    ~Pin() { if (s) unpin(s); }
    Pin(const Pin&) = delete;
    Pin& operator=(const Pin&) = delete;
};
struct ShardPin : Pin<Shard> { ShardPin(JNIEnv* env, jlong p) : Pin<Shard>(env, g_shards, p, "NativeSampler is closed") {} };
struct GroupPin : Pin<Group> { GroupPin(JNIEnv* env, jlong p) : Pin<Group>(env, g_groups, p, "group is closed") {} };

// close(): out of the registry under the lock, then wait for the calls that are still inside
template <class T>
T* unregister_and_drain(std::set<void*>& reg, jlong p)
{
    std::unique_lock<std::mutex> lk(g_reg_mutex);
    auto it = reg.find(reinterpret_cast<void*>(p));
    if (it == reg.end()) return nullptr;
    T* s = reinterpret_cast<T*>(*it);
    reg.erase(it);
    g_reg_cv.wait(lk, [&] { return s->pins == 0; });
    return s;
}

// RAII over Get/Release<Type>ArrayElements (mode 0: copy back and free; JNI_ABORT: input only)
// Several of them are declared side by side: once one Get has failed (OutOfMemoryError pending) the next ones take nothing -- JNI allows
// no Get while an exception is pending -- and report failed() as well.
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

}  // namespace mvhdp_jni

#endif  // MVHDP_JNI_COMMON_H
