// fake_jvm.cpp -- a test-side JNIEnv: the JNIEnv:: members tests/native/jni_stub/jni.h declares, defined here, so that the
// UNMODIFIED shim (mvtopicmodel_amd/java/mvhdp_jni.cpp) compiles against the stub header, links against this file and runs without
// a JVM.  Written from the JNI specification (chapter 4, "JNI Functions"), not from any JDK header.  It is strict where a real JVM
// is strict, and keeps a ledger of what a real JVM would punish silently or much later:
//   * Get<T>ArrayElements ALWAYS hands out a copy, between two guard blocks; Release with mode 0 copies back and frees, JNI_ABORT
//     frees only (so an output array released with JNI_ABORT loses its values, as it may in a JVM that copies);
//   * buffers never released, releases of pointers that are unknown or released already, damaged guards;
//   * local references: how many are outstanding when the native method returns, and the high-water mark (a JVM guarantees 16);
//   * region calls outside [0, length): ArrayIndexOutOfBoundsException, nothing transferred, counted;
//   * GetFieldID looks (name, signature) up in the field table the object's class was declared with: NoSuchFieldError and null;
//   * FindClass knows the exception classes only;
//   * every JNI call other than a release or DeleteLocalRef made while an exception is pending (but ExceptionCheck) is counted (the specification
//     forbids it); the pending exception, the ledger and the failure injection are per thread;
//   * the n-th Get<T>ArrayElements of a thread can be made to fail: null, OutOfMemoryError pending.
// The extern "C" surface fj_* at the end is what tests/jni_harness.py drives through ctypes.  Test infrastructure: never part of
// the product.
#include <jni.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace {

constexpr size_t GUARD = 32;                 // bytes either side of an elements buffer
constexpr unsigned char GUARD_BYTE = 0xA5;

struct FieldDecl { std::string name, sig; };
struct Klass { std::string name; std::vector<FieldDecl> fields; };
union Value { int64_t j; double d; };

// everything a jobject can point to; a local reference is an Obj of kind 'R' pointing at its target
struct Obj {
    char kind = 0;                           // 'I' 'J' 'D' 'Z' 'B': primitive arrays, 'L': object array, 'O': object, 'C': class, 'R': local reference
    int32_t length = 0;
    std::vector<unsigned char> data;         // primitive arrays
    std::vector<Obj*> elems;                 // object arrays
    Klass* klass = nullptr;                  // 'O': its class; 'C': the class itself
    std::vector<Value> values;               // 'O'
    Obj* target = nullptr;                   // 'R'
};

size_t elem_size(char kind)
{
    switch (kind) { case 'I': return 4; case 'J': case 'D': return 8; case 'Z': case 'B': return 1; default: return 0; }
}

const char* const KNOWN_CLASSES[] = {"java/lang/RuntimeException", "java/lang/IllegalArgumentException", "java/lang/IllegalStateException",
                                     "java/lang/OutOfMemoryError", "java/lang/ArrayIndexOutOfBoundsException", "java/lang/NoSuchFieldError",
                                     "java/lang/NoClassDefFoundError"};

std::mutex g_mutex;                          // the class table and the set of live objects (shared by all threads)
std::map<std::string, Klass*> g_classes;
std::set<Obj*> g_objects;

struct Buffer { Obj* array; unsigned char* base; size_t bytes; };

enum { L_BUFFERS_OUTSTANDING, L_BAD_RELEASES, L_GUARD_DAMAGE, L_LOCALS_LEFT, L_LOCAL_ARRAYS_LEFT, L_LOCALS_HIGH_WATER, L_REGION_OOB,
       L_CALLS_WHILE_PENDING, L_MISUSE, L_ELEMENTS_GETS, L_JNI_CALLS, L_COUNT };

struct Thread {
    bool pending = false;
    std::string exc_class, exc_msg;
    int64_t ledger[L_COUNT] = {};
    std::map<void*, Buffer> buffers;         // elements pointer -> its buffer
    std::set<Obj*> locals;
    int64_t fail_elements_at = 0;            // > 0: that Get<T>ArrayElements (counted from 1, from the moment it was set) fails
};
thread_local Thread T;

Klass* klass_of(const char* name)
{
    std::lock_guard<std::mutex> lk(g_mutex);
    auto it = g_classes.find(name);
    if (it != g_classes.end()) return it->second;
    Klass* k = new Klass();
    k->name = name;
    g_classes[name] = k;
    return k;
}

Obj* track(Obj* o) { std::lock_guard<std::mutex> lk(g_mutex); g_objects.insert(o); return o; }

void raise(const char* cls, const std::string& msg) { T.pending = true; T.exc_class = cls; T.exc_msg = msg; }

// every JNI function but the releases and DeleteLocalRef starts here
void enter() { T.ledger[L_JNI_CALLS]++; if (T.pending) T.ledger[L_CALLS_WHILE_PENDING]++; }

Obj* deref(const void* p)
{
    Obj* o = reinterpret_cast<Obj*>(const_cast<void*>(p));
    if (o && o->kind == 'R') o = o->target;
    return o;
}

// an object of the expected kind, or null with the misuse counted (a real JVM would crash or corrupt its heap)
Obj* expect(const void* p, char kind)
{
    Obj* o = deref(p);
    if (!o || o->kind != kind) { T.ledger[L_MISUSE]++; return nullptr; }
    return o;
}

Obj* expect_array(const void* p)
{
    Obj* o = deref(p);
    if (!o || !(elem_size(o->kind) || o->kind == 'L')) { T.ledger[L_MISUSE]++; return nullptr; }
    return o;
}

jobject new_local(Obj* target)
{
    Obj* r = new Obj();
    r->kind = 'R';
    r->target = target;
    T.locals.insert(r);
    if ((int64_t)T.locals.size() > T.ledger[L_LOCALS_HIGH_WATER]) T.ledger[L_LOCALS_HIGH_WATER] = (int64_t)T.locals.size();
    return reinterpret_cast<jobject>(r);
}

void* get_elements(const void* array, char kind, jboolean* is_copy)
{
    enter();
    T.ledger[L_ELEMENTS_GETS]++;
    Obj* a = expect(array, kind);
    if (!a) return nullptr;
    if (T.fail_elements_at > 0 && --T.fail_elements_at == 0) { raise("java/lang/OutOfMemoryError", "Get<Type>ArrayElements: injected"); return nullptr; }
    const size_t bytes = a->data.size();
    unsigned char* base = static_cast<unsigned char*>(std::malloc(bytes + 2 * GUARD));
    std::memset(base, GUARD_BYTE, GUARD);
    if (bytes) std::memcpy(base + GUARD, a->data.data(), bytes);
    std::memset(base + GUARD + bytes, GUARD_BYTE, GUARD);
    T.buffers[base + GUARD] = Buffer{a, base, bytes};
    T.ledger[L_BUFFERS_OUTSTANDING]++;
    if (is_copy) *is_copy = 1;
    return base + GUARD;
}

void release_elements(const void* array, char kind, void* p, jint mode)
{
    T.ledger[L_JNI_CALLS]++;                 // (allowed while an exception is pending)
    auto it = T.buffers.find(p);
    Obj* a = deref(array);
    if (it == T.buffers.end() || !a || a->kind != kind || it->second.array != a) { T.ledger[L_BAD_RELEASES]++; return; }
    Buffer b = it->second;
    bool damaged = false;
    for (size_t i = 0; i < GUARD; i++) damaged |= b.base[i] != GUARD_BYTE || b.base[GUARD + b.bytes + i] != GUARD_BYTE;
    if (damaged) T.ledger[L_GUARD_DAMAGE]++;
    if (mode != JNI_ABORT && b.bytes) std::memcpy(a->data.data(), b.base + GUARD, b.bytes);   // 0 and JNI_COMMIT (1) copy back
    if (mode == 1) return;                   // JNI_COMMIT: the buffer stays out
    T.buffers.erase(it);
    T.ledger[L_BUFFERS_OUTSTANDING]--;
    std::free(b.base);
}

// a region [start, start + len) of a primitive array of `kind`, or null: ArrayIndexOutOfBoundsException, nothing transferred
unsigned char* region(const void* array, char kind, jsize start, jsize len)
{
    enter();
    Obj* a = expect(array, kind);
    if (!a) return nullptr;
    if (start < 0 || len < 0 || (int64_t)start + len > a->length) {
        T.ledger[L_REGION_OOB]++;
        raise("java/lang/ArrayIndexOutOfBoundsException", "region " + std::to_string(start) + " + " + std::to_string(len) + " of an array of " + std::to_string(a->length));
        return nullptr;
    }
    return a->data.data() + (size_t)start * elem_size(kind);
}

void get_region(const void* array, char kind, jsize start, jsize len, void* buf)
{
    if (unsigned char* p = region(array, kind, start, len)) std::memcpy(buf, p, (size_t)len * elem_size(kind));
}

void set_region(const void* array, char kind, jsize start, jsize len, const void* buf)
{
    if (unsigned char* p = region(array, kind, start, len)) std::memcpy(p, buf, (size_t)len * elem_size(kind));
}

// the slot of field `fid` in object `obj` when the field is of that object's class and of signature `sig`
Value* field_slot(jobject obj, jfieldID fid, const char* sig)
{
    enter();
    Obj* o = expect(obj, 'O');
    if (!o) return nullptr;
    const FieldDecl* f = reinterpret_cast<const FieldDecl*>(fid);
    const FieldDecl* first = o->klass->fields.data();
    if (!f || f < first || f >= first + o->klass->fields.size() || f->sig != sig) { T.ledger[L_MISUSE]++; return nullptr; }
    return &o->values[(size_t)(f - first)];
}

JNIEnv g_env;

}  // namespace

// ---- the JNIEnv members of the stub header ----
jclass JNIEnv::FindClass(const char* name)
{
    enter();
    for (const char* k : KNOWN_CLASSES)
        if (!std::strcmp(k, name)) {
            Obj* c = new Obj();              // (owned by the local reference frame: freed with it)
            c->kind = 'C';
            c->klass = klass_of(name);
            jobject r = new_local(c);
            return reinterpret_cast<jclass>(r);
        }
    raise("java/lang/NoClassDefFoundError", name);
    return nullptr;
}

jint JNIEnv::ThrowNew(jclass cls, const char* msg)
{
    enter();
    Obj* c = expect(cls, 'C');
    if (!c) return -1;
    raise(c->klass->name.c_str(), msg ? msg : "");
    return 0;
}

jboolean JNIEnv::ExceptionCheck() { T.ledger[L_JNI_CALLS]++; return T.pending ? 1 : 0; }      // (allowed while an exception is pending)

jsize JNIEnv::GetArrayLength(jarray a)
{
    enter();
    Obj* o = expect_array(a);
    return o ? o->length : 0;
}

jobject JNIEnv::GetObjectArrayElement(jobjectArray a, jsize i)
{
    enter();
    Obj* o = expect(a, 'L');
    if (!o) return nullptr;
    if (i < 0 || i >= o->length) { T.ledger[L_REGION_OOB]++; raise("java/lang/ArrayIndexOutOfBoundsException", "element " + std::to_string(i)); return nullptr; }
    return o->elems[(size_t)i] ? new_local(o->elems[(size_t)i]) : nullptr;
}

void JNIEnv::DeleteLocalRef(jobject r)
{
    T.ledger[L_JNI_CALLS]++;                 // (allowed while an exception is pending)
    if (!r) return;                          // a null reference is a no-op
    Obj* o = reinterpret_cast<Obj*>(r);
    auto it = T.locals.find(o);
    if (it == T.locals.end()) { T.ledger[L_MISUSE]++; return; }
    T.locals.erase(it);
    if (o->target && o->target->kind == 'C') delete o->target;
    delete o;
}

jclass JNIEnv::GetObjectClass(jobject obj)
{
    enter();
    Obj* o = expect(obj, 'O');
    if (!o) return nullptr;
    Obj* c = new Obj();
    c->kind = 'C';
    c->klass = o->klass;
    return reinterpret_cast<jclass>(new_local(c));
}

jfieldID JNIEnv::GetFieldID(jclass cls, const char* name, const char* sig)
{
    enter();
    Obj* c = expect(cls, 'C');
    if (!c) return nullptr;
    for (const FieldDecl& f : c->klass->fields)
        if (f.name == name && f.sig == sig) return reinterpret_cast<jfieldID>(const_cast<FieldDecl*>(&f));
    raise("java/lang/NoSuchFieldError", std::string(name) + " " + sig);
    return nullptr;
}

void JNIEnv::SetLongField(jobject o, jfieldID f, jlong v) { if (Value* s = field_slot(o, f, "J")) s->j = v; }
void JNIEnv::SetIntField(jobject o, jfieldID f, jint v) { if (Value* s = field_slot(o, f, "I")) s->j = v; }
void JNIEnv::SetDoubleField(jobject o, jfieldID f, jdouble v) { if (Value* s = field_slot(o, f, "D")) s->d = v; }

jint* JNIEnv::GetIntArrayElements(jintArray a, jboolean* c) { return static_cast<jint*>(get_elements(a, 'I', c)); }
void JNIEnv::ReleaseIntArrayElements(jintArray a, jint* p, jint mode) { release_elements(a, 'I', p, mode); }
jlong* JNIEnv::GetLongArrayElements(jlongArray a, jboolean* c) { return static_cast<jlong*>(get_elements(a, 'J', c)); }
void JNIEnv::ReleaseLongArrayElements(jlongArray a, jlong* p, jint mode) { release_elements(a, 'J', p, mode); }
jdouble* JNIEnv::GetDoubleArrayElements(jdoubleArray a, jboolean* c) { return static_cast<jdouble*>(get_elements(a, 'D', c)); }
void JNIEnv::ReleaseDoubleArrayElements(jdoubleArray a, jdouble* p, jint mode) { release_elements(a, 'D', p, mode); }

void JNIEnv::GetIntArrayRegion(jintArray a, jsize s, jsize n, jint* b) { get_region(a, 'I', s, n, b); }
void JNIEnv::GetDoubleArrayRegion(jdoubleArray a, jsize s, jsize n, jdouble* b) { get_region(a, 'D', s, n, b); }
void JNIEnv::GetBooleanArrayRegion(jbooleanArray a, jsize s, jsize n, jboolean* b) { get_region(a, 'Z', s, n, b); }
void JNIEnv::GetLongArrayRegion(jlongArray a, jsize s, jsize n, jlong* b) { get_region(a, 'J', s, n, b); }
void JNIEnv::GetByteArrayRegion(jbyteArray a, jsize s, jsize n, jbyte* b) { get_region(a, 'B', s, n, b); }
void JNIEnv::SetDoubleArrayRegion(jdoubleArray a, jsize s, jsize n, const jdouble* b) { set_region(a, 'D', s, n, b); }
void JNIEnv::SetBooleanArrayRegion(jbooleanArray a, jsize s, jsize n, const jboolean* b) { set_region(a, 'Z', s, n, b); }
void JNIEnv::SetLongArrayRegion(jlongArray a, jsize s, jsize n, const jlong* b) { set_region(a, 'J', s, n, b); }
void JNIEnv::SetIntArrayRegion(jintArray a, jsize s, jsize n, const jint* b) { set_region(a, 'I', s, n, b); }
void JNIEnv::SetByteArrayRegion(jbyteArray a, jsize s, jsize n, const jbyte* b) { set_region(a, 'B', s, n, b); }

// ---- what the test drives (ctypes) ----
extern "C" {
#define FJ __attribute__((visibility("default")))

FJ void* fj_env(void) { return &g_env; }

// kind: 'I' int[], 'J' long[], 'D' double[], 'Z' boolean[], 'B' byte[], 'L' Object[]; zero-filled / null-filled
FJ void* fj_new_array(char kind, int32_t length)
{
    if (length < 0 || !(elem_size(kind) || kind == 'L')) return nullptr;
    Obj* o = new Obj();
    o->kind = kind;
    o->length = length;
    if (kind == 'L') o->elems.assign((size_t)length, nullptr);
    else o->data.assign((size_t)length * elem_size(kind), 0);
    return track(o);
}

FJ int32_t fj_array_length(void* a) { return static_cast<Obj*>(a)->length; }
FJ char fj_kind(void* a) { return static_cast<Obj*>(a)->kind; }
FJ void* fj_array_data(void* a) { return static_cast<Obj*>(a)->data.data(); }      // the Java heap's own storage of a primitive array
FJ void fj_set_object_element(void* a, int32_t i, void* v) { static_cast<Obj*>(a)->elems[(size_t)i] = static_cast<Obj*>(v); }

// fields: "name:sig,name:sig,..." -- the class is declared by its first object and must be declared the same way after that
FJ void* fj_new_object(const char* class_name, const char* fields)
{
    Klass* k = klass_of(class_name);
    std::vector<FieldDecl> decl;
    std::string s = fields ? fields : "";
    for (size_t at = 0; at < s.size();) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        const std::string item = s.substr(at, end - at);
        const size_t colon = item.find(':');
        if (colon == std::string::npos) return nullptr;
        decl.push_back(FieldDecl{item.substr(0, colon), item.substr(colon + 1)});
        at = end + 1;
    }
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        if (k->fields.empty()) k->fields = decl;
        else {
            if (k->fields.size() != decl.size()) return nullptr;
            for (size_t i = 0; i < decl.size(); i++) if (k->fields[i].name != decl[i].name || k->fields[i].sig != decl[i].sig) return nullptr;
        }
    }
    Obj* o = new Obj();
    o->kind = 'O';
    o->klass = k;
    o->values.assign(k->fields.size(), Value{0});
    return track(o);
}

static Value* named_field(void* obj, const char* name)
{
    Obj* o = static_cast<Obj*>(obj);
    for (size_t i = 0; i < o->klass->fields.size(); i++) if (o->klass->fields[i].name == name) return &o->values[i];
    return nullptr;
}
FJ int fj_has_field(void* obj, const char* name) { return named_field(obj, name) != nullptr; }
FJ int64_t fj_get_integral_field(void* obj, const char* name) { Value* v = named_field(obj, name); return v ? v->j : 0; }   // I and J fields
FJ double fj_get_double_field(void* obj, const char* name) { Value* v = named_field(obj, name); return v ? v->d : 0.0; }

FJ void fj_free(void* obj)
{
    Obj* o = static_cast<Obj*>(obj);
    { std::lock_guard<std::mutex> lk(g_mutex); if (!g_objects.erase(o)) return; }
    delete o;
}

FJ int64_t fj_live_objects(void) { std::lock_guard<std::mutex> lk(g_mutex); return (int64_t)g_objects.size(); }

// the pending exception of this thread: 1 and the two strings (valid until the next JNI call or clear), or 0
FJ int fj_exception(const char** cls, const char** msg)
{
    if (!T.pending) return 0;
    *cls = T.exc_class.c_str();
    *msg = T.exc_msg.c_str();
    return 1;
}
FJ void fj_exception_clear(void) { T.pending = false; T.exc_class.clear(); T.exc_msg.clear(); }

// a native method begins: a fresh local reference frame
FJ void fj_begin_call(void)
{
    T.ledger[L_LOCALS_HIGH_WATER] = 0;
    T.ledger[L_LOCALS_LEFT] = T.ledger[L_LOCAL_ARRAYS_LEFT] = 0;
}

// ... and returns: what is left in the frame is counted, then popped as a JVM pops it
FJ void fj_end_call(void)
{
    for (Obj* r : T.locals) {
        T.ledger[L_LOCALS_LEFT]++;
        if (r->target && r->target->kind == 'C') delete r->target; else T.ledger[L_LOCAL_ARRAYS_LEFT]++;
        delete r;
    }
    T.locals.clear();
}

FJ int fj_ledger_size(void) { return L_COUNT; }
FJ void fj_ledger(int64_t* out) { std::memcpy(out, T.ledger, sizeof T.ledger); }

// forgets the counters; buffers still out and local references still held are freed (a test that provoked a leak on purpose cleans up with this)
FJ void fj_ledger_reset(void)
{
    for (auto& kv : T.buffers) std::free(kv.second.base);
    T.buffers.clear();
    for (Obj* r : T.locals) { if (r->target && r->target->kind == 'C') delete r->target; delete r; }
    T.locals.clear();
    std::memset(T.ledger, 0, sizeof T.ledger);
    T.fail_elements_at = 0;
}

// the n-th Get<Type>ArrayElements of this thread from now on (n >= 1) returns null with OutOfMemoryError pending; 0: none
FJ void fj_fail_elements_at(int64_t n) { T.fail_elements_at = n; }

// self-tests of the fake: the JNI functions by hand, as a native method would call them
FJ void* fj_test_get_elements(void* a)
{
    switch (static_cast<Obj*>(a)->kind) {
    case 'I': return g_env.GetIntArrayElements(static_cast<jintArray>(a), nullptr);
    case 'J': return g_env.GetLongArrayElements(static_cast<jlongArray>(a), nullptr);
    case 'D': return g_env.GetDoubleArrayElements(static_cast<jdoubleArray>(a), nullptr);
    default: return nullptr;
    }
}
FJ void fj_test_release_elements(void* a, void* p, int32_t mode)
{
    switch (static_cast<Obj*>(a)->kind) {
    case 'I': g_env.ReleaseIntArrayElements(static_cast<jintArray>(a), static_cast<jint*>(p), mode); break;
    case 'J': g_env.ReleaseLongArrayElements(static_cast<jlongArray>(a), static_cast<jlong*>(p), mode); break;
    case 'D': g_env.ReleaseDoubleArrayElements(static_cast<jdoubleArray>(a), static_cast<jdouble*>(p), mode); break;
    default: break;
    }
}
FJ void fj_test_get_int_region(void* a, int32_t start, int32_t len, int32_t* buf) { g_env.GetIntArrayRegion(static_cast<jintArray>(a), start, len, buf); }
FJ void fj_test_set_int_region(void* a, int32_t start, int32_t len, const int32_t* buf) { g_env.SetIntArrayRegion(static_cast<jintArray>(a), start, len, buf); }
FJ int32_t fj_test_array_length(void* a) { return g_env.GetArrayLength(static_cast<jarray>(a)); }
FJ void* fj_test_object_element(void* a, int32_t i) { return g_env.GetObjectArrayElement(static_cast<jobjectArray>(a), i); }
FJ void fj_test_delete_local(void* r) { g_env.DeleteLocalRef(static_cast<jobject>(r)); }
FJ int fj_test_find_class(const char* name) { return g_env.FindClass(name) != nullptr; }
FJ int fj_test_throw(const char* cls, const char* msg) { jclass c = g_env.FindClass(cls); return c ? g_env.ThrowNew(c, msg) : -1; }
// 1: the field exists and was set; 0: GetFieldID refused it (NoSuchFieldError pending)
FJ int fj_test_set_long_field(void* obj, const char* name, const char* sig, int64_t v)
{
    jobject o = static_cast<jobject>(obj);
    jfieldID f = g_env.GetFieldID(g_env.GetObjectClass(o), name, sig);
    if (!f) return 0;
    if (!std::strcmp(sig, "J")) g_env.SetLongField(o, f, v);
    else if (!std::strcmp(sig, "I")) g_env.SetIntField(o, f, (jint)v);
    else g_env.SetDoubleField(o, f, (jdouble)v);
    return 1;
}

}  // extern "C"
