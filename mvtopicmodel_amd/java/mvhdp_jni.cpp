// mvhdp_jni.cpp — JNI shim between org.madgik.MVTopicModel.NativeSampler and the C ABI
// of libmvhdp.so (include/mvhdp.h).  NOT part of the build (no JDK there); a host builds it, with the three shim sources beside it, with
//   g++ -std=c++17 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude
//       mvtopicmodel_amd/java/mvhdp_jni.cpp mvtopicmodel_amd/java/mvhdp_sim_jni.cpp mvtopicmodel_amd/java/mvhdp_phrases_jni.cpp
//       mvtopicmodel_amd/java/mvhdp_heldout_jni.cpp -Lmvtopicmodel_amd/lib -lmvhdp -o libmvhdp_jni.so      (one command line)
// What the four sources share -- the handle registry, the pins, the exceptions, the array wrappers -- is mvhdp_jni_common.h.
// The tests compile the sources unmodified against a declaration-only jni.h (tests/native/jni_stub), link them against a test-side
// JNIEnv (tests/native/fake_jvm.cpp) and run every entry: tests/test_jni_fake_jvm.py without a device, tests/test_gpu_jni.py with one.
//
// Arrays cross with Get<Type>ArrayElements / Release<Type>ArrayElements, never with GetPrimitiveArrayCritical: every
// mvhdp_* call may block (hipMalloc, synchronous copies, a whole sweep), and JNI forbids blocking -- or any other JNI
// call -- inside a critical region (it stalls the collector for every Java thread and can deadlock it).  The elements
// calls may copy; the library copies once more into HBM, and the Java arrays are free to move meanwhile.  Every array
// length is checked against the shape the handle was created with before the library sees a pointer.
// A negative status becomes a RuntimeException carrying mvhdp_last_error().
#include <cstring>

#include "mvhdp_jni_common.h"

using mvhdp_jni::Shard; using mvhdp_jni::Group; using mvhdp_jni::ShardPin; using mvhdp_jni::GroupPin;
using mvhdp_jni::pin; using mvhdp_jni::unpin; using mvhdp_jni::unregister_and_drain;
using mvhdp_jni::g_reg_mutex; using mvhdp_jni::g_shards; using mvhdp_jni::g_groups;
using mvhdp_jni::throw_msg; using mvhdp_jni::throw_rt; using mvhdp_jni::bad_len;
using mvhdp_jni::Ints; using mvhdp_jni::Longs; using mvhdp_jni::Doubles;

extern "C" {

JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nCreate(JNIEnv* env, jclass, jint K, jintArray numTypes, jint device, jlong docIdBase)
{
    const jsize M = numTypes ? env->GetArrayLength(numTypes) : 0;
    if (M < 1 || M > MVHDP_MAX_MODALITIES) { throw_msg(env, "java/lang/IllegalArgumentException", "numTypes: 1..8 modalities"); return 0; }
    mvhdp_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.num_topics = K;
    cfg.num_modalities = M;
    env->GetIntArrayRegion(numTypes, 0, M, cfg.num_types);
    cfg.device = device;
    cfg.doc_id_base = docIdBase;
    Shard* s = new Shard();
    int rc = mvhdp_create(&cfg, &s->h);
    if (rc != MVHDP_OK) { delete s; throw_rt(env, nullptr, rc, "mvhdp_create"); return 0; }
    s->K = K; s->M = M;
    for (int m = 0; m < M; m++) s->V[m] = cfg.num_types[m];
    { std::lock_guard<std::mutex> lk(g_reg_mutex); g_shards.insert(s); }
    return reinterpret_cast<jlong>(s);
}

// Safe at any time, including from a finalizer or shutdown hook after the HIP runtime is gone (mvhdp_destroy then
// releases host memory only) and when called twice: the handle leaves the registry under the lock, a second call finds
// nothing and touches nothing.
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nDestroy(JNIEnv*, jclass, jlong p)
{
    Shard* s = unregister_and_drain<Shard>(g_shards, p);
    if (!s) return;
    mvhdp_destroy(s->h);
    delete s;
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetCorpus(JNIEnv* env, jclass, jlong p, jint m, jlongArray docOff, jintArray tokens)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M || !docOff || env->GetArrayLength(docOff) < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "setCorpus: bad view or docOff"); return; }
    const jsize D = env->GetArrayLength(docOff) - 1;
    int rc;
    jlong N = 0;
    {
        Longs o(env, docOff, JNI_ABORT);
        if (o.failed()) return;                                   // OutOfMemoryError pending
        N = o.p[D];
        if (N < 0 || (N > 0 && bad_len(env, tokens, N, "setCorpus tokens"))) return;
        Ints t(env, N > 0 ? tokens : nullptr, JNI_ABORT);
        if (t.failed()) return;
        rc = mvhdp_set_corpus(s->h, m, D, reinterpret_cast<const int64_t*>(o.p), reinterpret_cast<const int32_t*>(t.p));
    }
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_set_corpus"); return; }
    s->D = D; s->N[m] = N;
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetAssignments(JNIEnv* env, jclass, jlong p, jint m, jintArray z)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M) { throw_msg(env, "java/lang/IllegalArgumentException", "setAssignments: bad view"); return; }
    if (s->N[m] > 0 && bad_len(env, z, s->N[m], "setAssignments")) return;
    int rc;
    { Ints a(env, s->N[m] > 0 ? z : nullptr, JNI_ABORT); if (a.failed()) return;
      rc = mvhdp_set_assignments(s->h, m, reinterpret_cast<const int32_t*>(a.p)); }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_set_assignments");
}

// which entities HAVE the view (Assignments[m] != null) even when its FeatureSequence is empty: mvhdp_set_view_presence
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetViewPresence(JNIEnv* env, jclass, jlong p, jint m, jbooleanArray present)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M) { throw_msg(env, "java/lang/IllegalArgumentException", "setViewPresence: bad view"); return; }
    int rc;
    if (!present) rc = mvhdp_set_view_presence(s->h, m, nullptr);
    else {
        if (bad_len(env, present, s->D, "setViewPresence")) return;
        std::vector<uint8_t> v(static_cast<size_t>(s->D));
        env->GetBooleanArrayRegion(present, 0, (jsize)s->D, reinterpret_cast<jboolean*>(v.data()));
        rc = mvhdp_set_view_presence(s->h, m, v.data());
    }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_set_view_presence");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetAssignments(JNIEnv* env, jclass, jlong p, jint m, jintArray z)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M) { throw_msg(env, "java/lang/IllegalArgumentException", "getAssignments: bad view"); return; }
    if (s->N[m] == 0) return;
    if (bad_len(env, z, s->N[m], "getAssignments")) return;
    int rc;
    { Ints a(env, z, 0); if (a.failed()) return; rc = mvhdp_get_assignments(s->h, m, reinterpret_cast<int32_t*>(a.p)); }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_get_assignments");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetHyper(JNIEnv* env, jclass, jlong p, jobjectArray alpha, jdoubleArray alphaSum,
        jdoubleArray beta, jdoubleArray betaSum, jdoubleArray gamma, jobjectArray p_a, jobjectArray p_b, jbooleanArray inactive)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    const jsize M = s->M, K1 = s->K + 1;
    if (bad_len(env, alpha, M, "setHyper alpha") || bad_len(env, p_a, M, "setHyper p_a") || bad_len(env, p_b, M, "setHyper p_b") ||
        bad_len(env, alphaSum, M, "setHyper alphaSum") || bad_len(env, beta, M, "setHyper beta") ||
        bad_len(env, betaSum, M, "setHyper betaSum") || bad_len(env, gamma, M, "setHyper gamma")) return;
    if (inactive && bad_len(env, inactive, s->K, "setHyper inactive")) return;
    std::vector<double> a(static_cast<size_t>(M) * K1);
    mvhdp_hyper hy;
    std::memset(&hy, 0, sizeof hy);
    for (jsize m = 0; m < M; m++) {
        jdoubleArray r = static_cast<jdoubleArray>(env->GetObjectArrayElement(alpha, m));
        jdoubleArray pa = static_cast<jdoubleArray>(env->GetObjectArrayElement(p_a, m));
        jdoubleArray pb = static_cast<jdoubleArray>(env->GetObjectArrayElement(p_b, m));
        if (bad_len(env, r, K1, "setHyper alpha[m] (K+1 entries, PTM:196)") || bad_len(env, pa, M, "setHyper p_a[m]") || bad_len(env, pb, M, "setHyper p_b[m]")) {
            env->DeleteLocalRef(r); env->DeleteLocalRef(pa); env->DeleteLocalRef(pb);    // (a refusal leaves no row reference behind either)
            return;
        }
        env->GetDoubleArrayRegion(r, 0, K1, a.data() + static_cast<size_t>(m) * K1);
        env->GetDoubleArrayRegion(pa, 0, M, hy.p_a[m]);
        env->GetDoubleArrayRegion(pb, 0, M, hy.p_b[m]);
        env->DeleteLocalRef(r); env->DeleteLocalRef(pa); env->DeleteLocalRef(pb);
    }
    env->GetDoubleArrayRegion(alphaSum, 0, M, hy.alpha_sum);
    env->GetDoubleArrayRegion(beta, 0, M, hy.beta);
    env->GetDoubleArrayRegion(betaSum, 0, M, hy.beta_sum);
    env->GetDoubleArrayRegion(gamma, 0, M, hy.gamma);
    std::vector<uint8_t> ina;
    if (inactive) {
        ina.resize(static_cast<size_t>(s->K));
        env->GetBooleanArrayRegion(inactive, 0, s->K, reinterpret_cast<jboolean*>(ina.data()));
        hy.inactive = ina.data();
    }
    hy.alpha = a.data();
    int rc = mvhdp_set_hyper(s->h, &hy);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_set_hyper");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nBuildCounts(JNIEnv* env, jclass, jlong p)
{ ShardPin pin_(env, p); Shard* s = pin_.s; if (!s) return;
  int rc = mvhdp_build_counts(s->h); if (rc) throw_rt(env, s->h, rc, "mvhdp_build_counts"); }

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nBuildTrees(JNIEnv* env, jclass, jlong p)
{ ShardPin pin_(env, p); Shard* s = pin_.s; if (!s) return;
  int rc = mvhdp_build_trees(s->h); if (rc) throw_rt(env, s->h, rc, "mvhdp_build_trees"); }

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetCounts(JNIEnv* env, jclass, jlong p, jint m, jintArray nwk, jintArray nk)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M) { throw_msg(env, "java/lang/IllegalArgumentException", "getCounts: bad view"); return; }
    if ((nwk && bad_len(env, nwk, (jlong)s->V[m] * s->K, "getCounts typeTopicCounts")) || (nk && bad_len(env, nk, s->K, "getCounts tokensPerTopic"))) return;
    int rc;
    { Ints a(env, nwk, 0), b(env, nk, 0); if (a.failed() || b.failed()) return;
      rc = mvhdp_get_counts(s->h, m, reinterpret_cast<int32_t*>(a.p), reinterpret_cast<int32_t*>(b.p)); }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_get_counts");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetDocTopicHist(JNIEnv* env, jclass, jlong p, jint m, jintArray hist, jint histLen, jintArray lens)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M || histLen < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "getDocTopicHist: bad view or length"); return; }
    if (hist && bad_len(env, hist, (jlong)s->K * histLen, "getDocTopicHist hist")) return;
    int rc;
    { Ints a(env, hist, 0), b(env, lens, 0); if (a.failed() || b.failed()) return;
      rc = mvhdp_get_doc_topic_hist(s->h, m, reinterpret_cast<int32_t*>(a.p), histLen, reinterpret_cast<int32_t*>(b.p), lens ? env->GetArrayLength(lens) : 0); }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_get_doc_topic_hist");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetAlpha(JNIEnv* env, jclass, jlong p, jdoubleArray alphaFlat, jbooleanArray inactive)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, alphaFlat, (jlong)s->M * (s->K + 1), "getAlpha alpha") || bad_len(env, inactive, s->K, "getAlpha inactive")) return;
    std::vector<double> a(static_cast<size_t>(s->M) * (s->K + 1));
    std::vector<uint8_t> ina(static_cast<size_t>(s->K));
    int rc = mvhdp_get_alpha(s->h, a.data(), ina.data());
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_get_alpha"); return; }
    env->SetDoubleArrayRegion(alphaFlat, 0, (jsize)a.size(), a.data());
    env->SetBooleanArrayRegion(inactive, 0, s->K, reinterpret_cast<const jboolean*>(ina.data()));
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSweep(JNIEnv* env, jclass, jlong p, jint sweepIdx, jlong seed, jint flags, jdoubleArray pOverride, jobject out)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    // (D is -1 until setCorpus: there is no [D][M][M] to check against yet, and the library would refuse the sweep anyway)
    if (pOverride && s->D < 0) { throw_msg(env, "java/lang/IllegalStateException", "sweep pOverride: setCorpus has not been called"); return; }
    if (pOverride && bad_len(env, pOverride, s->D * static_cast<jlong>(s->M) * s->M, "sweep pOverride [D][M][M]")) return;
    mvhdp_sweep_stats st;
    int rc;
    {
        // the view weights are copied out first; the sweep itself runs with no Java array held
        std::vector<double> pcopy;
        if (pOverride) { pcopy.resize(static_cast<size_t>(env->GetArrayLength(pOverride))); env->GetDoubleArrayRegion(pOverride, 0, (jsize)pcopy.size(), pcopy.data()); }
        rc = mvhdp_sweep(s->h, static_cast<uint32_t>(sweepIdx), static_cast<uint64_t>(seed), static_cast<uint32_t>(flags),
                         pOverride ? pcopy.data() : nullptr, nullptr, &st);
    }
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_sweep"); return; }
    jclass c = env->GetObjectClass(out);
    auto setL = [&](const char* f, jlong v) { env->SetLongField(out, env->GetFieldID(c, f, "J"), v); };
    auto setI = [&](const char* f, jint v) { env->SetIntField(out, env->GetFieldID(c, f, "I"), v); };
    auto setD = [&](const char* f, jdouble v) { env->SetDoubleField(out, env->GetFieldID(c, f, "D"), v); };
    setL("tokens", st.tokens); setL("changed", st.changed); setL("newMassCnt", st.new_mass_cnt);
    setL("topicDocMassCnt", st.topic_doc_mass_cnt); setL("wordFTreeMassCnt", st.word_ftree_mass_cnt);
    setL("oovSkipped", st.oov_skipped); setL("abortedDocs", st.aborted_docs); setL("exactFallbacks", st.exact_fallbacks);
    setI("activatedTopic", st.activated_topic); setI("activatedModality", st.activated_modality);
    setL("activationKey", st.activation_key); setD("sweepKernelMs", st.sweep_kernel_ms); setD("totalMs", st.total_ms);
    setI("activations", st.activations);
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nApplyDelta(JNIEnv* env, jclass, jlong p, jint topic, jint modality)
{ ShardPin pin_(env, p); Shard* s = pin_.s; if (!s) return;
  int rc = mvhdp_apply_delta(s->h, topic, modality); if (rc) throw_rt(env, s->h, rc, "mvhdp_apply_delta"); }

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nModelLogLikelihood(JNIEnv* env, jclass, jlong p, jdoubleArray out)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, out, s->M, "modelLogLikelihood")) return;
    double ll[MVHDP_MAX_MODALITIES];
    int rc = mvhdp_model_log_likelihood(s->h, ll);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_model_log_likelihood"); return; }
    env->SetDoubleArrayRegion(out, 0, s->M, ll);
}

// statistics of n sweeps as a flat long array, 8 per sweep: tokens, changed, newMassCnt, topicDocMassCnt, wordFTreeMassCnt,
// oovSkipped, abortedDocs, exactFallbacks
static void stats_to_longs(const mvhdp_sweep_stats& st, jlong* o)
{
    o[0] = st.tokens; o[1] = st.changed; o[2] = st.new_mass_cnt; o[3] = st.topic_doc_mass_cnt;
    o[4] = st.word_ftree_mass_cnt; o[5] = st.oov_skipped; o[6] = st.aborted_docs; o[7] = st.exact_fallbacks;
}

// the iteration loop PTM:1146-1239 without a host round trip per iteration (mvhdp_sweep_many)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSweepMany(JNIEnv* env, jclass, jlong p, jint firstIdx, jint n, jlong seed, jint flags, jlongArray statsFlat)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (n < 0 || (statsFlat && bad_len(env, statsFlat, (jlong)n * 8, "sweepMany stats [n][8]"))) return;
    std::vector<mvhdp_sweep_stats> st(static_cast<size_t>(n > 0 ? n : 1));
    int rc = mvhdp_sweep_many(s->h, static_cast<uint32_t>(firstIdx), n, static_cast<uint64_t>(seed), static_cast<uint32_t>(flags), st.data());
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_sweep_many"); return; }
    if (statsFlat) {
        std::vector<jlong> flat(static_cast<size_t>(n) * 8);
        for (int i = 0; i < n; i++) stats_to_longs(st[i], flat.data() + (size_t)i * 8);
        env->SetLongArrayRegion(statsFlat, 0, (jsize)flat.size(), flat.data());
    }
}

// tuning block (mvhdp_tuning): ints = {forcePrimary, narrow, walkFixed, singleStream, live16, learntStep0, learntStep1, learntStep2},
// doubles = {primaryMinShare, walkTheta[8], treeBranchShare[8]}
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetTuning(JNIEnv* env, jclass, jlong p, jintArray ints, jdoubleArray doubles)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, ints, 8, "getTuning ints") || bad_len(env, doubles, 17, "getTuning doubles")) return;
    mvhdp_tuning t;
    int rc = mvhdp_get_tuning(s->h, &t);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_get_tuning"); return; }
    const jint iv[8] = {t.force_primary, t.narrow, t.walk_fixed, t.single_stream, t.live16, t.learnt_walk_step[0], t.learnt_walk_step[1], t.learnt_walk_step[2]};
    jdouble dv[17];
    dv[0] = t.primary_min_share;
    for (int m = 0; m < 8; m++) { dv[1 + m] = t.walk_theta[m]; dv[9 + m] = t.tree_branch_share[m]; }
    env->SetIntArrayRegion(ints, 0, 8, iv);
    env->SetDoubleArrayRegion(doubles, 0, 17, dv);
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetTuning(JNIEnv* env, jclass, jlong p, jintArray ints, jdoubleArray doubles)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, ints, 8, "setTuning ints") || bad_len(env, doubles, 17, "setTuning doubles")) return;
    jint iv[8]; jdouble dv[17];
    env->GetIntArrayRegion(ints, 0, 8, iv);
    env->GetDoubleArrayRegion(doubles, 0, 17, dv);
    // from the handle's own block: a field the Java block does not carry (single_wave, live_overlap, live_rows, whatever the struct
    // grows next) keeps the value the handle holds instead of being zeroed behind the host's back
    mvhdp_tuning t;
    int rc = mvhdp_get_tuning(s->h, &t);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_get_tuning"); return; }
    t.force_primary = iv[0]; t.narrow = iv[1]; t.walk_fixed = iv[2]; t.single_stream = iv[3]; t.live16 = iv[4];
    t.learnt_walk_step[0] = iv[5]; t.learnt_walk_step[1] = iv[6]; t.learnt_walk_step[2] = iv[7];
    t.primary_min_share = dv[0];
    for (int m = 0; m < 8; m++) { t.walk_theta[m] = dv[1 + m]; t.tree_branch_share[m] = dv[9 + m]; }
    rc = mvhdp_set_tuning(s->h, &t);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_set_tuning");
}

// ---- document shards on several GPUs: mvhdp_group_* (the reference's queue mesh + barrier, PTM:1042-1049, PTM:1232) ----
static void throw_group(JNIEnv* env, mvhdp_group g, int rc, const char* what)
{
    char msg[640];
    snprintf(msg, sizeof msg, "%s failed (%d): %s", what, rc, mvhdp_group_last_error(g));
    throw_msg(env, "java/lang/RuntimeException", msg);
}

// one JVM drives all its GPUs: one NativeSampler per device
JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupCreate(JNIEnv* env, jclass, jlongArray handles)
{
    const jsize n = handles ? env->GetArrayLength(handles) : 0;
    if (n < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "groupCreate: no members"); return 0; }
    std::vector<jlong> hp(static_cast<size_t>(n));
    env->GetLongArrayRegion(handles, 0, n, hp.data());
    std::vector<mvhdp_handle> hs;
    Group* gr = new Group();
    auto unpin_all = [&]() { for (Shard* s : gr->shards) unpin(s); gr->shards.clear(); };
    for (jsize i = 0; i < n; i++) {
        Shard* s = pin<Shard>(g_shards, hp[i]);
        if (!s) { unpin_all(); delete gr; throw_msg(env, "java/lang/IllegalStateException", "groupCreate: a member is closed"); return 0; }
        gr->shards.push_back(s);
        hs.push_back(s->h);
    }
    int rc = mvhdp_group_create(n, hs.data(), &gr->g);
    if (rc != MVHDP_OK) { unpin_all(); delete gr; throw_group(env, nullptr, rc, "mvhdp_group_create"); return 0; }
    gr->members = n; gr->K = gr->shards[0]->K; gr->M = gr->shards[0]->M;
    { std::lock_guard<std::mutex> lk(g_reg_mutex); g_groups.insert(gr); }
    return reinterpret_cast<jlong>(gr);
}

// one JVM per GPU: rank 0 makes the 128-byte id, the launcher hands it to the other ranks
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupUniqueId(JNIEnv* env, jclass, jbyteArray id)
{
    if (bad_len(env, id, MVHDP_UNIQUE_ID_BYTES, "groupUniqueId")) return;
    uint8_t buf[MVHDP_UNIQUE_ID_BYTES];
    int rc = mvhdp_group_unique_id(buf);
    if (rc) { throw_group(env, nullptr, rc, "mvhdp_group_unique_id"); return; }
    env->SetByteArrayRegion(id, 0, MVHDP_UNIQUE_ID_BYTES, reinterpret_cast<const jbyte*>(buf));
}

JNIEXPORT jlong JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupCreateRank(JNIEnv* env, jclass, jlong p, jbyteArray id, jint rank, jint nranks)
{
    Shard* s = pin<Shard>(g_shards, p);                           // (kept until nGroupDestroy)
    if (!s) { throw_msg(env, "java/lang/IllegalStateException", "NativeSampler is closed"); return 0; }
    if (bad_len(env, id, MVHDP_UNIQUE_ID_BYTES, "groupCreateRank id")) { unpin(s); return 0; }
    uint8_t buf[MVHDP_UNIQUE_ID_BYTES];
    env->GetByteArrayRegion(id, 0, MVHDP_UNIQUE_ID_BYTES, reinterpret_cast<jbyte*>(buf));
    Group* gr = new Group();
    int rc = mvhdp_group_create_rank(s->h, buf, rank, nranks, &gr->g);
    if (rc != MVHDP_OK) { unpin(s); delete gr; throw_group(env, nullptr, rc, "mvhdp_group_create_rank"); return 0; }
    gr->members = 1; gr->K = s->K; gr->M = s->M; gr->shards.push_back(s);
    { std::lock_guard<std::mutex> lk(g_reg_mutex); g_groups.insert(gr); }
    return reinterpret_cast<jlong>(gr);
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupDestroy(JNIEnv*, jclass, jlong p)
{
    Group* gr = unregister_and_drain<Group>(g_groups, p);
    if (!gr) return;
    mvhdp_group_destroy(gr->g);
    for (Shard* s : gr->shards) unpin(s);                         // the members may be closed now
    delete gr;
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupBuildCounts(JNIEnv* env, jclass, jlong p)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    int rc = mvhdp_group_build_counts(gr->g);
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_build_counts");
}

// statsFlat: [members][8] as nSweepMany; act: {activatedTopic, activatedModality, activations} of the sweep (the same on every replica);
// returns the device milliseconds of the exchange (collectives + updates + tree rebuilds)
JNIEXPORT jdouble JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupSweep(JNIEnv* env, jclass, jlong p, jint sweepIdx, jlong seed, jint flags, jlongArray statsFlat, jintArray act)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return 0.0;
    if ((statsFlat && bad_len(env, statsFlat, (jlong)gr->members * 8, "groupSweep stats [members][8]")) || (act && bad_len(env, act, 3, "groupSweep act"))) return 0.0;
    std::vector<mvhdp_sweep_stats> st(static_cast<size_t>(gr->members));
    int rc = mvhdp_group_sweep(gr->g, static_cast<uint32_t>(sweepIdx), static_cast<uint64_t>(seed), static_cast<uint32_t>(flags), st.data());
    if (rc) { throw_group(env, gr->g, rc, "mvhdp_group_sweep"); return 0.0; }
    if (statsFlat) {
        std::vector<jlong> flat(static_cast<size_t>(gr->members) * 8);
        for (int i = 0; i < gr->members; i++) stats_to_longs(st[i], flat.data() + (size_t)i * 8);
        env->SetLongArrayRegion(statsFlat, 0, (jsize)flat.size(), flat.data());
    }
    if (act) { const jint a[3] = {st[0].activated_topic, st[0].activated_modality, st[0].activations}; env->SetIntArrayRegion(act, 0, 3, a); }
    mvhdp_group_info info;
    return mvhdp_group_get_info(gr->g, &info) == MVHDP_OK ? info.last_exchange_ms : 0.0;
}

// ---- the steps either side of the sweep: one handle, and a sharded model (mvhdp_group_*) ----
// countHistogram of optimizeBeta PTM:2295-2309
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetCountHistogram(JNIEnv* env, jclass, jlong p, jint m, jintArray hist)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M || !hist || env->GetArrayLength(hist) < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "getCountHistogram: bad view or array"); return; }
    int rc;
    { Ints a(env, hist, 0); if (a.failed()) return; rc = mvhdp_get_count_histogram(s->h, m, reinterpret_cast<int32_t*>(a.p), env->GetArrayLength(hist)); }
    if (rc) throw_rt(env, s->h, rc, "mvhdp_get_count_histogram");
}

// optimizeP PTM:2706-2792: sums [M*M]
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nViewOverlapSums(JNIEnv* env, jclass, jlong p, jdoubleArray sums)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, sums, (jlong)s->M * s->M, "viewOverlapSums")) return;
    double v[MVHDP_MAX_MODALITIES * MVHDP_MAX_MODALITIES];
    int rc = mvhdp_view_overlap_sums(s->h, v);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_view_overlap_sums"); return; }
    env->SetDoubleArrayRegion(sums, 0, s->M * s->M, v);
}

// optimizeGamma's document level PTM:2415-2433: out = {qs, qw}
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGammaDocStatistics(JNIEnv* env, jclass, jlong p, jint m, jdouble gammaM, jlong seed, jint round, jdoubleArray out)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, out, 2, "gammaDocStatistics")) return;
    double v[2];
    int rc = mvhdp_gamma_doc_statistics(s->h, m, gammaM, static_cast<uint64_t>(seed), static_cast<uint32_t>(round), &v[0], &v[1]);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_gamma_doc_statistics"); return; }
    env->SetDoubleArrayRegion(out, 0, 2, v);
}

// optimizeDP's view-table simulation PTM:2454-2488: hist [K][histLen] (of the whole model), conc [K] = gamma[m] * alpha[m][t]; mk [K], active [K] filled
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nDpTableStatistics(JNIEnv* env, jclass, jlong p, jint m, jintArray hist, jint histLen, jdoubleArray conc,
                                                                                      jlong seed, jint round, jdoubleArray mk, jbyteArray active)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M || histLen < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "dpTableStatistics: bad view or histLen"); return; }
    if (bad_len(env, hist, (jlong)s->K * histLen, "dpTableStatistics hist [K][histLen]") || bad_len(env, conc, s->K, "dpTableStatistics conc") ||
        bad_len(env, mk, s->K, "dpTableStatistics mk") || bad_len(env, active, s->K, "dpTableStatistics active")) return;
    std::vector<double> cv(static_cast<size_t>(s->K)), mv(static_cast<size_t>(s->K));
    std::vector<uint8_t> av(static_cast<size_t>(s->K));
    env->GetDoubleArrayRegion(conc, 0, s->K, cv.data());
    int rc;
    { Ints a(env, hist, 0); if (a.failed()) return;
      rc = mvhdp_dp_table_statistics(s->h, m, reinterpret_cast<const int32_t*>(a.p), histLen, cv.data(), static_cast<uint64_t>(seed), static_cast<uint32_t>(round), mv.data(), av.data()); }
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_dp_table_statistics"); return; }
    env->SetDoubleArrayRegion(mk, 0, s->K, mv.data());
    env->SetByteArrayRegion(active, 0, s->K, reinterpret_cast<const jbyte*>(av.data()));
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupDrain(JNIEnv* env, jclass, jlong p)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    int rc = mvhdp_group_drain(gr->g);
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_drain");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupAbort(JNIEnv* env, jclass, jlong p)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    int rc = mvhdp_group_abort(gr->g);
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_abort");
}

// modelLogLikelihood PTM:3322-3452 of the sharded model: out [M]
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupModelLogLikelihood(JNIEnv* env, jclass, jlong p, jdoubleArray out)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    if (bad_len(env, out, gr->M, "groupModelLogLikelihood: one entry per view")) return;
    double ll[MVHDP_MAX_MODALITIES] = {};
    int rc = mvhdp_group_log_likelihood(gr->g, ll);
    if (rc) { throw_group(env, gr->g, rc, "mvhdp_group_log_likelihood"); return; }
    env->SetDoubleArrayRegion(out, 0, env->GetArrayLength(out), ll);
}

// topicDocCounts / docLengthCounts over every entity of every member: hist [K*histLen]
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupGetDocTopicHist(JNIEnv* env, jclass, jlong p, jint m, jintArray hist, jint histLen, jintArray lens)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    // (the library zero-fills and sums K * histLen entries whatever it is handed: the shape is checked HERE, against the members' K and M)
    if (m < 0 || m >= gr->M || histLen < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "groupGetDocTopicHist: bad view or histLen"); return; }
    if (hist && bad_len(env, hist, (jlong)gr->K * histLen, "groupGetDocTopicHist hist [K][histLen]")) return;
    int rc;
    { Ints a(env, hist, 0), b(env, lens, 0); if (a.failed() || b.failed()) return;
      rc = mvhdp_group_doc_topic_hist(gr->g, m, reinterpret_cast<int32_t*>(a.p), histLen, reinterpret_cast<int32_t*>(b.p), lens ? env->GetArrayLength(lens) : 0); }
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_doc_topic_hist");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupGetCountHistogram(JNIEnv* env, jclass, jlong p, jint m, jintArray hist)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    if (m < 0 || m >= gr->M || !hist || env->GetArrayLength(hist) < 1) { throw_msg(env, "java/lang/IllegalArgumentException", "groupGetCountHistogram: bad view or empty array"); return; }
    int rc;
    { Ints a(env, hist, 0); if (a.failed()) return; rc = mvhdp_group_count_histogram(gr->g, m, reinterpret_cast<int32_t*>(a.p), env->GetArrayLength(hist)); }
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_count_histogram");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupViewOverlapSums(JNIEnv* env, jclass, jlong p, jdoubleArray sums)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    const jsize n = gr->M * gr->M;
    if (bad_len(env, sums, n, "groupViewOverlapSums [M][M]")) return;
    double v[MVHDP_MAX_MODALITIES * MVHDP_MAX_MODALITIES] = {};
    int rc = mvhdp_group_view_overlap_sums(gr->g, v);
    if (rc) { throw_group(env, gr->g, rc, "mvhdp_group_view_overlap_sums"); return; }
    env->SetDoubleArrayRegion(sums, 0, n, v);
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupGammaDocStatistics(JNIEnv* env, jclass, jlong p, jint m, jdouble gammaM, jlong seed, jint round, jdoubleArray out)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    if (m < 0 || m >= gr->M) { throw_msg(env, "java/lang/IllegalArgumentException", "groupGammaDocStatistics: bad view"); return; }
    if (bad_len(env, out, 2, "groupGammaDocStatistics")) return;
    double v[2];
    int rc = mvhdp_group_gamma_doc_statistics(gr->g, m, gammaM, static_cast<uint64_t>(seed), static_cast<uint32_t>(round), &v[0], &v[1]);
    if (rc) { throw_group(env, gr->g, rc, "mvhdp_group_gamma_doc_statistics"); return; }
    env->SetDoubleArrayRegion(out, 0, 2, v);
}

// ---- topic diagnostics (FastQMVWVTopicModelDiagnostics; include/mvhdp.h mvhdp_top_words / mvhdp_discr_weights / mvhdp_diagnostics) ----
// getSortedWords(m) PTM:1792-1811 cut at n: typesFlat / counts [K*n] (unfilled: -1 / 0), nonzero [K]
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nTopWords(JNIEnv* env, jclass, jlong p, jint m, jint n, jintArray types, jintArray counts, jintArray nonzero)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (n < 1 || n > MVHDP_DIAG_MAX_TOP_WORDS) { throw_msg(env, "java/lang/IllegalArgumentException", "topWords: n must be 1..64"); return; }
    if (bad_len(env, types, (jlong)s->K * n, "topWords types") || bad_len(env, counts, (jlong)s->K * n, "topWords counts") || bad_len(env, nonzero, s->K, "topWords nonzero")) return;
    Ints t(env, types, 0), c(env, counts, 0), z(env, nonzero, 0);
    if (t.failed() || c.failed() || z.failed()) return;
    int rc = mvhdp_top_words(s->h, m, n, t.p, c.p, z.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_top_words");
}

// calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230: perView [M] = discrWeightPerModality; typeWeight [V_m] or null
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nDiscrWeights(JNIEnv* env, jclass, jlong p, jdoubleArray perView, jint m, jdoubleArray typeWeight)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (m < 0 || m >= s->M) { throw_msg(env, "java/lang/IllegalArgumentException", "discrWeights: bad view"); return; }
    if (bad_len(env, perView, s->M, "discrWeights perView") || (typeWeight && bad_len(env, typeWeight, s->V[m], "discrWeights typeWeight"))) return;
    Doubles pv(env, perView, 0), tw(env, typeWeight, 0);
    if (pv.failed() || tw.failed()) return;
    int rc = mvhdp_discr_weights(s->h, pv.p, m, tw.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_discr_weights");
}

// the arrays of one mvhdp_diag_out, checked against the shape: scores [13*K], wordScores [13*K*n], codoc [K*n*n], topTypes / topCounts
// [K*n], nonzero / rank1Docs / nonzeroDocs [K], atProportions [K*7], sumCountLogCount [K], wordTypeCounts [V_0], numTokens [1], perView [M]
namespace {                          // (file-private: a type made of the hidden namespace's cannot be more visible than they are)
struct DiagArrays {
    Doubles scores, wordScores; Ints codoc, topTypes, topCounts, nonzero, rank1, nzDocs, props; Doubles scl; Ints wtc; Longs ntok; Doubles perView;
    Ints wl;
    bool failed() const
    {
        return scores.failed() || wordScores.failed() || codoc.failed() || topTypes.failed() || topCounts.failed() || nonzero.failed() || rank1.failed() ||
               nzDocs.failed() || props.failed() || scl.failed() || wtc.failed() || ntok.failed() || perView.failed() || wl.failed();
    }
    void fill(mvhdp_diag_args& a, mvhdp_diag_out& o, jint n) const
    {
        a.num_top_words = n; a.word_length = wl.p;
        o.scores = scores.p; o.word_scores = wordScores.p; o.codoc = codoc.p; o.top_types = topTypes.p; o.top_counts = topCounts.p;
        o.nonzero = nonzero.p; o.num_rank1_docs = rank1.p; o.num_nonzero_docs = nzDocs.p; o.num_docs_at_proportions = props.p;
        o.sum_count_log_count = scl.p; o.word_type_counts = wtc.p; o.num_tokens = (int64_t*)ntok.p; o.discr_weight_per_view = perView.p;
    }
};
}  // namespace

static bool bad_diag(JNIEnv* env, jint K, jint M, jint V0, jint n, jintArray wordLength, jdoubleArray scores, jdoubleArray wordScores, jintArray codoc,
                     jintArray topTypes, jintArray topCounts, jintArray nonzero, jintArray rank1, jintArray nzDocs, jintArray props, jdoubleArray scl,
                     jintArray wtc, jlongArray ntok, jdoubleArray perView)
{
    if (n < 1 || n > MVHDP_DIAG_MAX_TOP_WORDS) { throw_msg(env, "java/lang/IllegalArgumentException", "diagnostics: numTopWords must be 1..64"); return true; }
    const jlong k = K, nn = n;
    return (wordLength && bad_len(env, wordLength, V0, "diagnostics wordLength")) || bad_len(env, scores, MVHDP_DIAG_ROWS * k, "diagnostics scores") ||
           bad_len(env, wordScores, MVHDP_DIAG_ROWS * k * nn, "diagnostics wordScores") || bad_len(env, codoc, k * nn * nn, "diagnostics codoc") ||
           bad_len(env, topTypes, k * nn, "diagnostics topTypes") || bad_len(env, topCounts, k * nn, "diagnostics topCounts") ||
           bad_len(env, nonzero, k, "diagnostics nonzero") || bad_len(env, rank1, k, "diagnostics rank1Docs") || bad_len(env, nzDocs, k, "diagnostics nonzeroDocs") ||
           bad_len(env, props, k * MVHDP_DIAG_PROPORTIONS, "diagnostics atProportions") || bad_len(env, scl, k, "diagnostics sumCountLogCount") ||
           bad_len(env, wtc, V0, "diagnostics wordTypeCounts") || bad_len(env, ntok, 1, "diagnostics numTokens") || bad_len(env, perView, M, "diagnostics perView");
}

#define DIAG_PARAMS jint n, jintArray wordLength, jdoubleArray scores, jdoubleArray wordScores, jintArray codoc, jintArray topTypes, jintArray topCounts, \
    jintArray nonzero, jintArray rank1, jintArray nzDocs, jintArray props, jdoubleArray scl, jintArray wtc, jlongArray ntok, jdoubleArray perView
#define DIAG_ARRAYS DiagArrays da{{env, scores, 0}, {env, wordScores, 0}, {env, codoc, 0}, {env, topTypes, 0}, {env, topCounts, 0}, {env, nonzero, 0}, \
    {env, rank1, 0}, {env, nzDocs, 0}, {env, props, 0}, {env, scl, 0}, {env, wtc, 0}, {env, ntok, 0}, {env, perView, 0}, {env, wordLength, JNI_ABORT}}

// FastQMVWVTopicModelDiagnostics(model, n) DIAG:53-117 on the device (getSortedWords + collectDocumentStatistics + the score rows)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nDiagnostics(JNIEnv* env, jclass, jlong p, DIAG_PARAMS)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_diag(env, s->K, s->M, s->V[0], n, wordLength, scores, wordScores, codoc, topTypes, topCounts, nonzero, rank1, nzDocs, props, scl, wtc, ntok, perView)) return;
    DIAG_ARRAYS;
    if (da.failed()) return;
    mvhdp_diag_args a{}; mvhdp_diag_out o{};
    da.fill(a, o, n);
    int rc = mvhdp_diagnostics(s->h, &a, &o);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_diagnostics");
}

// the same for the sharded model (mvhdp_group_diagnostics; collective across processes)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGroupDiagnostics(JNIEnv* env, jclass, jlong p, DIAG_PARAMS)
{
    GroupPin gpin_(env, p); Group* gr = gpin_.s;
    if (!gr) return;
    if (gr->shards.empty()) { throw_msg(env, "java/lang/IllegalStateException", "group has no member"); return; }
    if (bad_diag(env, gr->K, gr->M, gr->shards[0]->V[0], n, wordLength, scores, wordScores, codoc, topTypes, topCounts, nonzero, rank1, nzDocs, props, scl, wtc, ntok, perView)) return;
    DIAG_ARRAYS;
    if (da.failed()) return;
    mvhdp_diag_args a{}; mvhdp_diag_out o{};
    da.fill(a, o, n);
    int rc = mvhdp_group_diagnostics(gr->g, &a, &o);
    if (rc) throw_group(env, gr->g, rc, "mvhdp_group_diagnostics");
}

// ---- word and topic embeddings (TopicWordEmbeddings TWE / TopicWordEmbeddingRunnable TWER; include/mvhdp.h mvhdp_emb_*) ----
// Every array is flat and checked against the embedding shape the handle was given by nEmbInit: [R*C] vectors (R = V_0, + K with
// topics), [V_0] word statistics, [K*V_0] softmax, [n] nearest.  null where the header allows it.
static bool emb_missing(JNIEnv* env, const Shard* s)
{
    if (s->embR > 0) return false;
    throw_msg(env, "java/lang/IllegalStateException", "embeddings: embInit has not been called");
    return true;
}

// new TopicWordEmbeddings(alphabet[0], C, Cc, window, K, ..) TWE:126-163: ints {numColumns, numContextColumns, withTopics, window,
// numSamples, minDocLength, sigmoidCacheSize}, doubles {samplingFactor, minExp, maxExp}; weights [R*C] or null (drawn on the device)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbInit(JNIEnv* env, jclass, jlong p, jintArray ints, jlong tableSize, jdoubleArray doubles, jdoubleArray weights, jlong seed)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, ints, 7, "embInit ints") || bad_len(env, doubles, 3, "embInit doubles")) return;
    jint iv[7]; jdouble dv[3];
    env->GetIntArrayRegion(ints, 0, 7, iv);
    env->GetDoubleArrayRegion(doubles, 0, 3, dv);
    mvhdp_emb_config c;
    std::memset(&c, 0, sizeof c);
    c.num_columns = iv[0]; c.num_context_columns = iv[1]; c.with_topics = iv[2] ? 1 : 0; c.window = iv[3]; c.num_samples = iv[4];
    c.min_doc_length = iv[5]; c.sigmoid_cache_size = iv[6]; c.sampling_table_size = tableSize;
    c.sampling_factor = dv[0]; c.min_exp = dv[1]; c.max_exp = dv[2];
    const jlong R = (jlong)s->V[0] + (c.with_topics ? s->K : 0);
    if (weights && (c.num_columns < 1 || bad_len(env, weights, R * c.num_columns, "embInit weights [R*C]"))) return;
    Doubles w(env, weights, JNI_ABORT);
    if (w.failed()) return;
    int rc = mvhdp_emb_init(s->h, &c, w.p, static_cast<uint64_t>(seed));
    // a refused configuration (MVHDP_ERR_INVALID_ARG) is refused before the library touches the embedding it holds: that one, and its
    // shape here, stand; any later failure has freed it
    if (rc) { if (rc != MVHDP_ERR_INVALID_ARG) { s->embR = 0; s->embC = 0; s->embK = 0; } throw_rt(env, s->h, rc, "mvhdp_emb_init"); return; }
    s->embR = R; s->embC = c.num_columns; s->embK = c.with_topics ? s->K : 0;
}

// countWords(data, f) TWE:341-401 (cumulative, as the reference's)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbCountWords(JNIEnv* env, jclass, jlong p)
{ ShardPin pin_(env, p); Shard* s = pin_.s; if (!s) return;
  int rc = mvhdp_emb_count_words(s->h); if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_count_words"); }

// train(data, threads, numSamples, epochs) TWE:423-483: longs [7] {wordsSoFar, wordsSampled, wordsConsidered, docsSkipped, calls,
// negativesSkipped, lastEpochCalls}, doubles [3] {residual, lastEpochResidual, kernelMs}
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbTrain(JNIEnv* env, jclass, jlong p, jint epochs, jlong seed, jint round, jint flags, jlongArray longs, jdoubleArray doubles)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (bad_len(env, longs, 7, "embTrain longs") || bad_len(env, doubles, 3, "embTrain doubles")) return;
    mvhdp_emb_stats st;
    std::memset(&st, 0, sizeof st);
    int rc = mvhdp_emb_train(s->h, epochs, static_cast<uint64_t>(seed), static_cast<uint32_t>(round), static_cast<uint32_t>(flags), &st);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_emb_train"); return; }
    const jlong l[7] = {st.words_so_far, st.words_sampled, st.words_considered, st.docs_skipped, st.calls, st.negatives_skipped, st.last_epoch_calls};
    const jdouble d[3] = {st.residual, st.last_epoch_residual, st.kernel_ms};
    env->SetLongArrayRegion(longs, 0, 7, l);
    env->SetDoubleArrayRegion(doubles, 0, 3, d);
}

// getWordVectors / getTopicVectors TWE:726-745 (rows V_0.. are the topics): [R*C] each, or null
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbGetVectors(JNIEnv* env, jclass, jlong p, jdoubleArray weights, jdoubleArray negativeWeights)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    const jlong n = s->embR * s->embC;
    if ((weights && bad_len(env, weights, n, "embGetVectors weights")) || (negativeWeights && bad_len(env, negativeWeights, n, "embGetVectors negativeWeights"))) return;
    Doubles w(env, weights, 0), g(env, negativeWeights, 0);
    if (w.failed() || g.failed()) return;
    int rc = mvhdp_emb_get_vectors(s->h, w.p, g.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_get_vectors");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbSetVectors(JNIEnv* env, jclass, jlong p, jdoubleArray weights, jdoubleArray negativeWeights)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    const jlong n = s->embR * s->embC;
    if ((weights && bad_len(env, weights, n, "embSetVectors weights")) || (negativeWeights && bad_len(env, negativeWeights, n, "embSetVectors negativeWeights"))) return;
    Doubles w(env, weights, JNI_ABORT), g(env, negativeWeights, JNI_ABORT);
    if (w.failed() || g.failed()) return;
    int rc = mvhdp_emb_set_vectors(s->h, w.p, g.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_set_vectors");
}

// wordCounts [V_0], retentionProbability [V_0] (either may be null), totalWords [1]
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbWordStats(JNIEnv* env, jclass, jlong p, jlongArray counts, jdoubleArray retention, jlongArray totalWords)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    if ((counts && bad_len(env, counts, s->V[0], "embWordStats counts")) || (retention && bad_len(env, retention, s->V[0], "embWordStats retention")) ||
        bad_len(env, totalWords, 1, "embWordStats totalWords")) return;
    Longs c(env, counts, 0);
    Doubles r(env, retention, 0);
    if (c.failed() || r.failed()) return;
    int64_t total = 0;
    int rc = mvhdp_emb_word_stats(s->h, reinterpret_cast<int64_t*>(c.p), r.p, &total);
    if (rc) { throw_rt(env, s->h, rc, "mvhdp_emb_word_stats"); return; }
    const jlong t = total;
    env->SetLongArrayRegion(totalWords, 0, 1, &t);
}

// samplingTable[first .. first + types.length)
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbSamplingTable(JNIEnv* env, jclass, jlong p, jlong first, jintArray types)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    if (!types) { throw_msg(env, "java/lang/IllegalArgumentException", "embSamplingTable: types is null"); return; }
    Ints t(env, types, 0);
    if (t.failed()) return;
    int rc = mvhdp_emb_sampling_table(s->h, first, env->GetArrayLength(types), t.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_sampling_table");
}

// CalcSoftmaxTopicWordProbabilities PTM:337-367: expDotProductValues [K*V_0] or null, sumExpValues [K] (accumulated, PTM:360) or null
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbSoftmax(JNIEnv* env, jclass, jlong p, jboolean resetSums, jdoubleArray expDot, jdoubleArray sumExp)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    if ((expDot && bad_len(env, expDot, (jlong)s->embK * s->V[0], "embSoftmax expDot [K*V_0]")) || (sumExp && bad_len(env, sumExp, s->embK, "embSoftmax sumExp"))) return;
    Doubles e(env, expDot, 0), m(env, sumExp, 0);
    if (e.failed() || m.failed()) return;
    int rc = mvhdp_emb_softmax(s->h, resetSums ? 1 : 0, e.p, m.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_softmax");
}

// findClosest TWE:485-540: query [C]; words / wordSims [n]; topics / topicSims [n] or null
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbNearest(JNIEnv* env, jclass, jlong p, jdoubleArray query, jint n, jintArray words, jdoubleArray wordSims, jintArray topics, jdoubleArray topicSims)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if (emb_missing(env, s)) return;
    if (n < 1 || n > 64) { throw_msg(env, "java/lang/IllegalArgumentException", "embNearest: n must be 1..64"); return; }
    if (bad_len(env, query, s->embC, "embNearest query") || bad_len(env, words, n, "embNearest words") || bad_len(env, wordSims, n, "embNearest wordSims") ||
        (topics && bad_len(env, topics, n, "embNearest topics")) || (topicSims && bad_len(env, topicSims, n, "embNearest topicSims"))) return;
    Doubles q(env, query, JNI_ABORT), ws(env, wordSims, 0), ts(env, topicSims, 0);
    Ints w(env, words, 0), t(env, topics, 0);
    if (q.failed() || ws.failed() || ts.failed() || w.failed() || t.failed()) return;
    int rc = mvhdp_emb_nearest(s->h, q.p, n, w.p, ws.p, t.p, ts.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_emb_nearest");
}

JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nEmbRelease(JNIEnv* env, jclass, jlong p)
{ ShardPin pin_(env, p); Shard* s = pin_.s; if (!s) return;
  int rc = mvhdp_emb_release(s->h); if (rc) { throw_rt(env, s->h, rc, "mvhdp_emb_release"); return; } s->embR = 0; s->embC = 0; s->embK = 0; }

// useVectorsLambda (PTM:1199-1207): lambda = 0 switches the mix off; expDot [K*V_0] / sumExp [K] in the reference's layout, or both null:
// the handle's own softmax table as the last embSoftmax left it
JNIEXPORT void JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nSetVectorsMix(JNIEnv* env, jclass, jlong p, jdouble lambda, jdoubleArray expDot, jdoubleArray sumExp)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return;
    if ((expDot == nullptr) != (sumExp == nullptr)) { throw_msg(env, "java/lang/IllegalArgumentException", "setVectorsMix: expDot and sumExp go together"); return; }
    if ((expDot && bad_len(env, expDot, (jlong)s->K * s->V[0], "setVectorsMix expDot [K*V_0]")) || (sumExp && bad_len(env, sumExp, s->K, "setVectorsMix sumExp"))) return;
    Doubles e(env, expDot, JNI_ABORT), m(env, sumExp, JNI_ABORT);
    if (e.failed() || m.failed()) return;
    int rc = mvhdp_set_vectors_mix(s->h, lambda, e.p, m.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_set_vectors_mix");
}

// returns lambda (0: off); mix [V_0*K] or null: lambda * (e / S) as the device holds it
JNIEXPORT jdouble JNICALL Java_org_madgik_MVTopicModel_NativeSampler_nGetVectorsMix(JNIEnv* env, jclass, jlong p, jdoubleArray mix)
{
    ShardPin pin_(env, p); Shard* s = pin_.s;
    if (!s) return 0.0;
    if (mix && bad_len(env, mix, (jlong)s->V[0] * s->K, "getVectorsMix mix [V_0*K]")) return 0.0;
    Doubles t(env, mix, 0);
    if (t.failed()) return 0.0;
    double lambda = 0.0;
    int rc = mvhdp_get_vectors_mix(s->h, &lambda, t.p);
    if (rc) throw_rt(env, s->h, rc, "mvhdp_get_vectors_mix");
    return lambda;
}

}  // extern "C"
