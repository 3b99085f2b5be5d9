// mvhdp_api.hip — host side of the C ABI declared in include/mvhdp.h.
// Owns the device state of one model shard (one HIP device), launches the
// kernels of mvhdp_kernels.hip on one stream and copies results back.
// There is NO CPU fallback: without a gfx950 device mvhdp_create fails.
#include "mvhdp_side.h"                      // check_offsets (set_corpus)

static thread_local std::string g_create_error;

// ---- handle registry and process exit ------------------------------------------------------------------
// Every live handle is listed here.  The first mvhdp_create registers an atexit handler; it is registered AFTER the
// HIP runtime initialised (hipGetDeviceCount in mvhdp_create comes first), so at exit it runs BEFORE the runtime's own
// teardown: it releases the device resources of every handle still open and marks the process as exiting.  A host that
// closes a handle later than that -- a JVM finalizer or shutdown hook calling NativeSampler.close(), a static destructor
// of the embedding program -- reaches mvhdp_destroy with g_exiting set: no HIP call is made any more, only host memory is
// released.  mvhdp_destroy of a pointer that is not (or no longer) a live handle is refused instead of dereferenced.
static std::mutex g_reg_mutex;
static std::set<mvhdp_ctx*>* g_live = nullptr;          // heap-allocated and never freed: usable during static destruction
static bool g_exiting = false, g_atexit_registered = false;
static void release_device_resources(mvhdp_ctx* h);

static void mvhdp_at_exit()
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    g_exiting = true;
    if (g_live) for (mvhdp_ctx* h : *g_live) release_device_resources(h);     // the runtime is still alive here
}

static void register_handle(mvhdp_ctx* h)
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    if (!g_live) g_live = new std::set<mvhdp_ctx*>();
    g_live->insert(h);
    if (!g_atexit_registered) { atexit(mvhdp_at_exit); g_atexit_registered = true; }
}

bool mvhdp_is_live(mvhdp_ctx* h)
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    return g_live && g_live->count(h) != 0;
}

// The environment is read ONCE, here (diagnostics; a host uses mvhdp_set_tuning):
//   MVHDP_FORCE_RMAX=1|2|4|8|16   primary variant          MVHDP_NARROW=0        never the 16-bit mirror
//   MVHDP_WALK_THETA=t0,t1,...    fixed walk thresholds    MVHDP_SINGLE_STREAM=1 class kernels one after another
//   MVHDP_DEBUG=1                 the plan of every sweep on stderr
//   MVHDP_OVERLAP_SERIAL, MVHDP_NO_ROW_SAMPLE, MVHDP_NO_HEAVY_REFRESH (set, whatever the value): measurement switches, mvhdp_ctx::Diag
// (a -DMVHDP_PROBE build alone reads one more per sweep, MVHDP_ATOMIC_PROBE: tools/mode_times.py changes it between the sweeps of one handle)
static void read_environment(mvhdp_ctx* h)
{
    if (const char* f = getenv("MVHDP_FORCE_RMAX")) { const int v = atoi(f); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32) h->tu.force_primary = v; }
    if (const char* f = getenv("MVHDP_NARROW")) h->tu.narrow = atoi(f) != 0 ? -1 : 0;
    if (const char* f = getenv("MVHDP_SINGLE_STREAM")) h->tu.single_stream = atoi(f) != 0;
    if (const char* f = getenv("MVHDP_SIDE_PRIORITY")) h->side_priority = atoi(f);               // 0: none, 1: A, B and D, 2 (default): A and B      // 0: every side stream at normal priority (diagnostics)
    if (const char* f = getenv("MVHDP_LIVE16")) h->tu.live16 = atoi(f);
    if (const char* f = getenv("MVHDP_LIVE_OVERLAP")) h->tu.live_overlap = atoi(f);
    if (const char* f = getenv("MVHDP_LIVE_ROWS")) h->tu.live_rows = atoi(f);                     // 0: stored trees rebuilt at every segment border (the round-4 form of a live sweep)
    if (const char* f = getenv("MVHDP_LIVE_ROWS_THETA")) h->tu.live_rows_theta = atof(f);
    if (const char* f = getenv("MVHDP_COEF_LDS_KB")) h->tu.coef_lds_max_bytes = std::max(0, std::min(64, atoi(f))) * 1024;   // (experiment: the live-rows coefficient table in LDS up to this size)
    if (const char* f = getenv("MVHDP_LIVE_ROWS_SEGMENTS")) h->tu.live_rows_segments = std::max(1, std::min(255, atoi(f)));
    if (const char* f = getenv("MVHDP_WIDEST_ON_MAIN")) h->tu.widest_on_main = atoi(f) != 0;
    if (const char* f = getenv("MVHDP_NARROW_WIDE")) h->tu.narrow_wide = atoi(f) != 0;
    if (const char* f = getenv("MVHDP_SLIM")) h->tu.slim = std::max(0, std::min(2, atoi(f)));    // 0: no 12-bit image of n_wk (A/B runs); 2: wherever its rows have fewer lines than the mirror's
    if (const char* f = getenv("MVHDP_LIVE_TREE_EVERY")) h->live_tree_every = std::max(1, atoi(f));   // (diagnostics: a live sweep rebuilds its trees at every n-th segment border only)
    if (const char* f = getenv("MVHDP_GATE_PCT")) { const int v = atoi(f); if (v >= 5 && v <= 95) h->gate_pct = v; }   // how far through a live segment the next one is prepared
    if (const char* f = getenv("MVHDP_FOUR_ROUND_ON_C")) h->tu.four_round_on_c = atoi(f);         // -1 by its token share (default), 0 / 1
    if (const char* f = getenv("MVHDP_DELTA16")) h->tu.delta16 = atoi(f) != 0;                   // 0: every n_wk delta in the 32-bit table (diagnostics)
    if (const char* f = getenv("MVHDP_FORK_DELAY_US")) h->tu.fork_delay_us = std::max(0, std::min(1000, atoi(f)));
    if (const char* f = getenv("MVHDP_FORCE_MODE")) { if (!strcmp(f, "serial")) h->tu.single_stream = 1; }   // "streams" (default): class kernels side by side
    if (const char* f = getenv("MVHDP_PRIMARY_MIN_SHARE")) { const double v = atof(f); if (v > 0.0 && v <= 1.0) h->tu.primary_min_share = v; }
    if (const char* t = getenv("MVHDP_WALK_THETA")) {
        int m = 0;
        for (const char* q = t; *q && m < MVHDP_MAXM; m++) {
            h->tu.walk_theta[m] = atof(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        for (; m < MVHDP_MAXM; m++) h->tu.walk_theta[m] = 0.0;
        h->tu.walk_fixed = 1;
    }
    h->dbg_env = getenv("MVHDP_DEBUG") != nullptr;
    h->diag.overlap_serial = getenv("MVHDP_OVERLAP_SERIAL") != nullptr;
    h->diag.no_row_sample = getenv("MVHDP_NO_ROW_SAMPLE") != nullptr;
    h->diag.no_heavy_refresh = getenv("MVHDP_NO_HEAVY_REFRESH") != nullptr;
}

hipError_t make_stream(hipStream_t* out, bool high_priority)
{
    int least = 0, greatest = 0;
    if (high_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least &&
        hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest) == hipSuccess) return hipSuccess;
    if (high_priority) { (void)hipGetLastError(); *out = nullptr; }  // (a runtime without stream priorities, or whose range query fails: an ordinary stream then)
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

extern "C" const char* mvhdp_version(void) { return "mvhdp 0.1 (gfx950)"; }

extern "C" const char* mvhdp_last_error(mvhdp_handle h) { return (h && mvhdp_is_live(h)) ? h->err.c_str() : g_create_error.c_str(); }

extern "C" int mvhdp_create(const mvhdp_config* cfg, mvhdp_handle* out)
{
    if (!cfg || !out) { g_create_error = "null argument"; return MVHDP_ERR_INVALID_ARG; }
    *out = nullptr;
    const int K = cfg->num_topics, M = cfg->num_modalities;
    if (K < 1 || K > MVHDP_MAX_TOPICS || M < 1 || M > MVHDP_MAX_MODALITIES) {
        g_create_error = "num_topics must be in [1,2048] and num_modalities in [1,8]";
        return MVHDP_ERR_INVALID_ARG;
    }
    for (int m = 0; m < M; m++) if (cfg->num_types[m] < 1) { g_create_error = "num_types[m] must be >= 1"; return MVHDP_ERR_INVALID_ARG; }
    for (int m = 0; m < M; m++) if (cfg->num_types[m] >= (1 << 29)) { g_create_error = "num_types[m] must be below 2^29"; return MVHDP_ERR_INVALID_ARG; }
    if (cfg->doc_id_base < 0 || cfg->doc_id_base >= (1LL << 29)) { g_create_error = "doc_id_base out of range"; return MVHDP_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_error = "no usable HIP device (the sweep has no CPU fallback)";
        return MVHDP_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return MVHDP_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return MVHDP_ERR_NO_DEVICE;
    }
    mvhdp_ctx* h = new mvhdp_ctx();
    register_handle(h);
    h->cfg = *cfg;
    h->device = cfg->device;
    h->num_cus = prop.multiProcessorCount;
    h->max_lds = 160 * 1024;
    MvModel& mm = h->mm;
    mm.K = K; mm.M = M;
    mm.rowbase[0] = 0;
    for (int m = 0; m < M; m++) { mm.V[m] = cfg->num_types[m]; mm.rowbase[m + 1] = mm.rowbase[m] + cfg->num_types[m]; }
    mm.doc_id_base = cfg->doc_id_base;
    mm.first_inactive = -1;
    mm.D = -1;
#define CREATE_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    g_create_error = std::string(#call) + ": " + hipGetErrorString(e_); mvhdp_destroy(h); return MVHDP_ERR_HIP; } } while (0)
    CREATE_HIP(hipSetDevice(h->device));
    CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    for (auto& e : h->ev) CREATE_HIP(hipEventCreate(&e));
    const int64_t nrows = mm.rowbase[M];
    // (+ MVHDP_TAIL_WORDS behind the tokensPerTopic part of both buffers: the status word a group of document shards reduces together
    // with that part, so that every rank learns of a failure on any rank inside the collective it has to enter anyway)
    const size_t cbytes = (size_t)(nrows * K + (int64_t)M * K + MVHDP_TAIL_WORDS) * sizeof(int32_t);
    CREATE_HIP(hipMalloc(&mm.counts, cbytes));
    CREATE_HIP(hipMalloc(&mm.delta, cbytes));
    CREATE_HIP(hipMemset(mm.counts, 0, cbytes));
    CREATE_HIP(hipMalloc(&mm.counts16, (size_t)nrows * K * sizeof(uint16_t) + 64));   // (+ 64: the 16-byte row loads of the live-rows form may end beyond the last row)
    CREATE_HIP(hipMemset(mm.counts16, 0, (size_t)nrows * K * sizeof(uint16_t)));
    CREATE_HIP(hipMalloc(&mm.delta16, (size_t)(nrows * K + 2) * sizeof(uint16_t)));
    CREATE_HIP(hipMemsetD16(mm.delta16, (unsigned short)0x8000, (size_t)(nrows * K + 2)));       // (the bias: see SweepLaunch::delta16)
    CREATE_HIP(hipMalloc(&mm.heavy, (size_t)nrows));
    CREATE_HIP(hipMemset(mm.heavy, 1, (size_t)nrows));
    CREATE_HIP(hipMemset(mm.delta, 0, cbytes));
    CREATE_HIP(hipMalloc(&mm.trees, (size_t)nrows * 2 * K * sizeof(double)));
    CREATE_HIP(hipMalloc(&mm.root, (size_t)nrows * sizeof(double)));
    CREATE_HIP(hipMalloc(&mm.mass0, (size_t)nrows * sizeof(float)));
    CREATE_HIP(hipMemset(mm.mass0, 0, (size_t)nrows * sizeof(float)));
    CREATE_HIP(hipMalloc(&mm.coef, (size_t)M * (((K + 7) & ~7) + K + 8) * sizeof(float)));   // coef [M][Kp] (zero-padded rows), then the smoothing running sums [M][K]
    {
        // descent table layout (MvModel::dtab): internal levels nlev, first block dt_f levels, then blocks of three
        const int nlev = (K > 1) ? (32 - __builtin_clz((unsigned)(K - 1))) : 0;
        mm.dt_f = nlev ? ((nlev - 1) % 3) + 1 : 0;
        mm.dt_nbd = 1; mm.dt_base[0] = 0; mm.dt_depth[0] = 0;
        int nblk = 1;
        for (int dep = mm.dt_f; nlev && dep < nlev; dep += 3) {
            mm.dt_base[mm.dt_nbd] = nblk; mm.dt_depth[mm.dt_nbd] = dep; mm.dt_nbd++;
            nblk += 1 << dep;
        }
        mm.dt_nblk = nblk;
        CREATE_HIP(hipMalloc(&mm.dtab, (size_t)nrows * nblk * 8 * sizeof(double)));
    }
    CREATE_HIP(hipMalloc(&h->d_alpha, (size_t)M * (K + 1) * sizeof(double)));
    CREATE_HIP(hipMalloc(&h->d_inactive, (size_t)K));
    CREATE_HIP(hipMemset(h->d_inactive, 0, (size_t)K));
    CREATE_HIP(hipMalloc(&h->d_births, (size_t)(2 + 2 * K) * sizeof(int32_t)));
    CREATE_HIP(hipMemset(h->d_births, 0, (size_t)(2 + 2 * K) * sizeof(int32_t)));
    CREATE_HIP(hipMalloc(&h->d_birth_keys, (size_t)K * sizeof(long long)));
    CREATE_HIP(hipMalloc(&h->d_birth_table, (size_t)K * sizeof(long long)));
    {
        const std::vector<long long> none((size_t)K, LLONG_MAX);                       // MVHDP_BUF_BIRTH_KEYS before any sweep: nothing born
        CREATE_HIP(hipMemcpy(h->d_birth_table, none.data(), (size_t)K * sizeof(long long), hipMemcpyHostToDevice));
    }
    CREATE_HIP(hipMalloc(&h->d_ctl, CTL_WORDS * sizeof(unsigned long long)));
    CREATE_HIP(hipMemset(h->d_ctl, 0, CTL_WORDS * sizeof(unsigned long long)));
    h->d_stats = h->d_ctl;
    h->d_act_key = (long long*)(h->d_ctl + ST_COUNT);
    h->d_ovf_meta = (unsigned int*)(h->d_ctl + ST_COUNT + 1);
    h->d_doc_counter = h->d_ctl + ST_COUNT + 1 + META_WORDS64;                       // one work-queue head per kernel class
    CREATE_HIP(hipHostMalloc((void**)&h->h_ctl, CTL_WORDS * sizeof(unsigned long long), hipHostMallocDefault));   // pinned: the read-back never blocks the host
    for (int c = 0; c < MVHDP_N_CLASSES; c++)
        for (int f = 0; f < MVHDP_N_FLAVOURS; f++) { h->regs.regs[c][f] = mvhdp_sweep_kernel_regs(c, f); h->regs.regs_mix[c][f] = mvhdp_sweep_kernel_regs(c, f == MVHDP_FLAVOUR_PLAIN ? MVHDP_FLAVOUR_WALK : f, true); }
    read_environment(h);
    {
        // the 12-bit image of n_wk (mvhdp_slim.h): only where a plan can use it (38 MB at C4)
        int vmax = 0;
        for (int m = 0; m < M; m++) vmax = std::max(vmax, (int)cfg->num_types[m]);
        if (plan_slim_table(K, vmax, h->tu.slim)) {
            CREATE_HIP(hipMalloc(&mm.counts12, (size_t)nrows * mvhdp_slim_row_bytes(K)));
            CREATE_HIP(hipMemset(mm.counts12, 0, (size_t)nrows * mvhdp_slim_row_bytes(K)));
        }
    }
    mm.alpha = h->d_alpha;
    mm.inactive = h->d_inactive;
    h->h_alpha.assign((size_t)M * (K + 1), 0.0);
    h->h_inactive.assign((size_t)K, 0);
    h->wt.init_defaults(K);
    h->wt_mix.init_defaults(K);
    *out = h;
    return MVHDP_OK;
}

// frees everything the handle holds on the device; idempotent (every pointer is cleared)
static void release_device_resources(mvhdp_ctx* h)
{
    if (h->device_released) return;
    h->device_released = true;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    auto fr = [](auto*& p) { if (p) { hipFree((void*)p); p = nullptr; } };
    for (int m = 0; m < MVHDP_MAXM; m++) { fr(h->d_doc_off[m]); fr(h->d_tok[m]); fr(h->d_z[m]); fr(h->d_carry[m]); fr(h->d_present[m]); }
    fr(h->mm.counts); fr(h->mm.delta16); fr(h->mm.counts16); fr(h->mm.counts12); fr(h->mm.heavy); fr(h->mm.delta); fr(h->mm.trees); fr(h->mm.root); fr(h->mm.coef); fr(h->mm.mass0); fr(h->d_births); fr(h->d_birth_keys); fr(h->d_birth_table); fr(h->mm.dtab); fr(h->mm.p);
    fr(h->d_alpha); fr(h->d_inactive); fr(h->d_ctl);
    fr(h->d_mix); fr(h->d_mix32); h->mm.mix = nullptr; h->mm.mix32 = nullptr; h->mix_lambda = 0.0;
    mvhdp_emb_free(h);
    if (h->h_ctl) { hipHostFree(h->h_ctl); h->h_ctl = nullptr; }
    h->d_stats = nullptr; h->d_act_key = nullptr; h->d_doc_counter = nullptr; h->d_ovf_meta = nullptr;
    fr(h->d_doc_order); fr(h->d_lists); fr(h->d_nslots); fr(h->d_stats_many); fr(h->d_heavy_list); fr(h->d_heavy_ctl);
    fr(h->census.d_blocks); fr(h->census.d_tally); h->census.on = false;
    if (h->ev_rf_go) { hipEventDestroy(h->ev_rf_go); h->ev_rf_go = nullptr; }
    if (h->ev_rf_done) { hipEventDestroy(h->ev_rf_done); h->ev_rf_done = nullptr; }
    if (h->rf_stream) { hipStreamDestroy(h->rf_stream); h->rf_stream = nullptr; }
    fr(h->ov.counts2); fr(h->ov.counts16_2); fr(h->ov.dtab2); fr(h->ov.root2); fr(h->ov.trees2); fr(h->ov.delta2); fr(h->ov.delta3); fr(h->ov.ctl2); fr(h->ov.lists2);
    for (auto& e : h->ov.ev_seg) if (e) { hipEventDestroy(e); e = nullptr; }
    if (h->ov.ev_start) { hipEventDestroy(h->ov.ev_start); h->ov.ev_start = nullptr; }
    if (h->ov.x1) { hipStreamDestroy(h->ov.x1); h->ov.x1 = nullptr; }
    if (h->ov.xa) { hipStreamDestroy(h->ov.xa); h->ov.xa = nullptr; }
    for (auto& e : h->ev_many) if (e) { hipEventDestroy(e); e = nullptr; }
    for (auto& e : h->ev) if (e) { hipEventDestroy(e); e = nullptr; }
    if (h->ev_fork) { hipEventDestroy(h->ev_fork); h->ev_fork = nullptr; }
    for (auto& e : h->ev_join) if (e) { hipEventDestroy(e); e = nullptr; }
    for (auto& st : h->side) if (st) { hipStreamDestroy(st); st = nullptr; }
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    h->stream = nullptr;
}

extern "C" int mvhdp_destroy(mvhdp_handle h)
{
    if (!h) return MVHDP_OK;
    bool exiting;
    {
        std::lock_guard<std::mutex> lk(g_reg_mutex);
        if (!g_live || g_live->erase(h) == 0) return MVHDP_ERR_INVALID_ARG;      // not a live handle (closed twice?)
        exiting = g_exiting;
    }
    // after the exit handler has run the HIP runtime may be gone: it released the device side already, touch nothing
    if (!exiting) release_device_resources(h);
    delete h;
    return MVHDP_OK;
}

extern "C" int mvhdp_set_stream(mvhdp_handle h, void* hip_stream)
{
    CHECK_H(h);
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->own_stream) { hipStreamDestroy(h->stream); h->own_stream = false; }
    if (hip_stream) h->stream = (hipStream_t)hip_stream;
    else { HIPC(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    return MVHDP_OK;
}

extern "C" int mvhdp_synchronize(mvhdp_handle h)
{
    CHECK_H(h);
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

extern "C" int mvhdp_set_corpus(mvhdp_handle h, int32_t m, int64_t D, const int64_t* doc_off, const int32_t* tokens)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M || D < 0 || !doc_off) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_corpus: bad view, num_docs or doc_off");
    if (mm.D >= 0 && D != mm.D) {
        bool any_other = false;
        for (int j = 0; j < mm.M; j++) if (j != m && h->have_corpus[j]) any_other = true;
        if (any_other) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_corpus: every view must list the same entities (empty span = view absent)");
    }
    if (mm.doc_id_base + D >= (1LL << 29)) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_corpus: too many entities");
    if (const char* r = check_offsets(doc_off, D, (1 << 20) - 1)) FAIL(h, MVHDP_ERR_INVALID_ARG, std::string("set_corpus: doc_off (a view of one entity: at most 2^20 - 1 tokens) ") + r);
    const int64_t N = doc_off[D];
    if (N > 0 && !tokens) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_corpus: tokens is null");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->d_doc_off[m]) { hipFree(h->d_doc_off[m]); h->d_doc_off[m] = nullptr; }
    if (h->d_tok[m]) { hipFree(h->d_tok[m]); h->d_tok[m] = nullptr; }
    if (h->d_z[m]) { hipFree(h->d_z[m]); h->d_z[m] = nullptr; }
    if (h->d_present[m]) { hipFree(h->d_present[m]); h->d_present[m] = nullptr; }
    h->h_present[m].clear(); mm.present[m] = nullptr;
    HIPC(h, hipMalloc(&h->d_doc_off[m], (size_t)(D + 1) * sizeof(int64_t)));
    HIPC(h, hipMemcpy(h->d_doc_off[m], doc_off, (size_t)(D + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    const size_t nb = (size_t)std::max<int64_t>(N, 1) * sizeof(int32_t);
    HIPC(h, hipMalloc(&h->d_tok[m], nb));
    HIPC(h, hipMalloc(&h->d_z[m], nb));
    if (N > 0) HIPC(h, hipMemcpy(h->d_tok[m], tokens, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(h, hipMemset(h->d_z[m], 0xff, nb));               // UNASSIGNED_TOPIC (-1), PTM:63
    h->h_doc_off[m].assign(doc_off, doc_off + D + 1);
    h->N[m] = N;
    h->have_corpus[m] = true;
    h->max_doc_tokens = -1;
    if (h->d_doc_order) { hipFree(h->d_doc_order); h->d_doc_order = nullptr; }
    if (h->d_lists) { hipFree(h->d_lists); h->d_lists = nullptr; }
    if (h->ov.lists2) { hipFree(h->ov.lists2); h->ov.lists2 = nullptr; }
    if (h->d_nslots) { hipFree(h->d_nslots); h->d_nslots = nullptr; }
    mm.nslots = nullptr;
    for (auto& c : h->d_carry) if (c) { hipFree(c); c = nullptr; }
    mm.D = D;
    mm.doc_off[m] = (const int64_t*)h->d_doc_off[m];
    mm.tok[m] = (const int32_t*)h->d_tok[m];
    mm.z[m] = (int32_t*)h->d_z[m];
    if (mm.p) { hipFree(mm.p); mm.p = nullptr; }
    h->st.corpus_replaced(m, N > 0);
    return MVHDP_OK;
}

int require_corpus(mvhdp_ctx* h)
{
    for (int m = 0; m < h->mm.M; m++)
        if (!h->have_corpus[m]) FAIL(h, MVHDP_ERR_STATE, "set_corpus has not been called for every view");
    return MVHDP_OK;
}

extern "C" int mvhdp_set_assignments(mvhdp_handle h, int32_t m, const int32_t* z)
{
    CHECK_H(h);
    if (m < 0 || m >= h->mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_assignments: bad view");
    if (!h->have_corpus[m]) FAIL(h, MVHDP_ERR_STATE, "set_assignments before set_corpus");
    if (h->N[m] > 0 && !z) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_assignments: null z");
    bool any_unassigned = false;
    for (int64_t i = 0; i < h->N[m]; i++) {
        if (z[i] < -1 || z[i] >= h->mm.K) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_assignments: topic out of range");
        any_unassigned = any_unassigned || z[i] < 0;
    }
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->N[m] > 0) HIPC(h, hipMemcpy(h->d_z[m], z, (size_t)h->N[m] * sizeof(int32_t), hipMemcpyHostToDevice));
    // the counts no longer describe these assignments: a sampling sweep is refused until build_counts / set_counts /
    // counts_written says they do again (a frozen sweep, whose counts are a trained model's by design, is not)
    h->st.assignments_replaced(m, any_unassigned);
    return MVHDP_OK;
}

extern "C" int mvhdp_set_view_presence(mvhdp_handle h, int32_t m, const uint8_t* present)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_view_presence: bad view");
    if (!h->have_corpus[m]) FAIL(h, MVHDP_ERR_STATE, "set_view_presence before set_corpus");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->d_present[m]) { hipFree(h->d_present[m]); h->d_present[m] = nullptr; }
    h->h_present[m].clear(); mm.present[m] = nullptr;
    if (h->d_carry[m]) { hipFree(h->d_carry[m]); h->d_carry[m] = nullptr; }         // the carry-over map of doc_topic_proportions depends on it
    if (!present || mm.D == 0) return MVHDP_OK;
    for (int64_t d = 0; d < mm.D; d++)
        if (!present[d] && h->h_doc_off[m][d + 1] > h->h_doc_off[m][d]) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_view_presence: an entity with tokens in the view is marked absent");
    h->h_present[m].assign(present, present + mm.D);
    HIPC(h, hipMalloc(&h->d_present[m], (size_t)mm.D));
    HIPC(h, hipMemcpy(h->d_present[m], present, (size_t)mm.D, hipMemcpyHostToDevice));
    mm.present[m] = h->d_present[m];
    return MVHDP_OK;
}

extern "C" int mvhdp_get_assignments(mvhdp_handle h, int32_t m, int32_t* z)
{
    CHECK_H(h);
    if (m < 0 || m >= h->mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_assignments: bad view");
    if (!h->have_corpus[m]) FAIL(h, MVHDP_ERR_STATE, "get_assignments before set_corpus");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->N[m] > 0) HIPC(h, hipMemcpy(z, h->d_z[m], (size_t)h->N[m] * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_set_hyper(mvhdp_handle h, const mvhdp_hyper* hy)
{
    CHECK_H(h);
    if (!hy || !hy->alpha) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_hyper: null");
    MvModel& mm = h->mm;
    const int K = mm.K, M = mm.M;
    for (int m = 0; m < M; m++) {
        // (n_wk+beta)/(n_k+betaSum) is evaluated with the unscaled IEEE division sequence (div_inrange):
        // keep both operands far from the exponent limits
        if (!(hy->beta_sum[m] >= 1e-30 && hy->beta_sum[m] <= 1e30) || !(hy->beta[m] >= 1e-30 && hy->beta[m] <= 1e30))
            FAIL(h, MVHDP_ERR_INVALID_ARG, "set_hyper: beta and beta_sum must be in [1e-30, 1e30]");
        mm.alpha_sum[m] = hy->alpha_sum[m]; mm.beta[m] = hy->beta[m];
        mm.beta_sum[m] = hy->beta_sum[m];   mm.gamma[m] = hy->gamma[m];
        for (int j = 0; j < M; j++) { mm.p_a[m][j] = hy->p_a[m][j]; mm.p_b[m][j] = hy->p_b[m][j]; }
    }
    h->h_alpha.assign(hy->alpha, hy->alpha + (size_t)M * (K + 1));
    if (hy->inactive) h->h_inactive.assign(hy->inactive, hy->inactive + K);
    else h->h_inactive.assign((size_t)K, 0);
    mm.first_inactive = -1;
    for (int k = 0; k < K; k++) if (h->h_inactive[k]) { mm.first_inactive = k; break; }
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipMemcpy(h->d_alpha, h->h_alpha.data(), (size_t)M * (K + 1) * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMemcpy(h->d_inactive, h->h_inactive.data(), (size_t)K, hipMemcpyHostToDevice));
    h->have_hyper = true;
    h->st.trees_outdated();
    return MVHDP_OK;
}

extern "C" int mvhdp_get_alpha(mvhdp_handle h, double* alpha, uint8_t* inactive)
{
    CHECK_H(h);
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "get_alpha before set_hyper");
    if (alpha) memcpy(alpha, h->h_alpha.data(), h->h_alpha.size() * sizeof(double));
    if (inactive) memcpy(inactive, h->h_inactive.data(), h->h_inactive.size());
    return MVHDP_OK;
}

extern "C" int mvhdp_build_counts(mvhdp_handle h)
{
    CHECK_H(h);
    int rc = require_corpus(h); if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, mvhdp_launch_build_counts(h->mm, h->N, h->stream));
    if (h->st.delta_pending()) {
        // a NO_APPLY sweep's deltas were never applied: z already holds its assignments, so the recount above includes
        // them -- drop the deltas instead of leaving them to be added on top
        HIPC(h, hipMemsetAsync(h->mm.delta, 0, (size_t)counts_len(h) * sizeof(int32_t), h->stream));
        h->st.delta_zeroed();
    }
    if (h->st.delta16_used()) {
        // 16-bit delta cells of a sweep that never reached its apply pass (it failed: the recount is how a host recovers): back to the bias
        HIPC(h, hipMemsetD16Async(h->mm.delta16, (unsigned short)0x8000, (size_t)(h->mm.rowbase[h->mm.M] * h->mm.K), h->stream));
        h->st.delta16_rebiased();
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.counts_rebuilt();
    return MVHDP_OK;
}

// The trees are current (trees_current) but the last sweep refreshed only the descent table: write the FTree.tree
// arrays as well, from the same counts and hyper-parameters (nothing has changed them since, or trees_current were false).
static int ensure_full_trees(mvhdp_ctx* h)
{
    if (!h->st.trees_current() || h->st.full_trees()) return MVHDP_OK;
    HIPC(h, mvhdp_launch_build_trees(h->mm, h->st.trees_inference(), true, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.full_trees_written();
    return MVHDP_OK;
}

extern "C" int mvhdp_build_trees(mvhdp_handle h)
{
    CHECK_H(h);
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "build_trees before set_hyper");
    if (!h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "build_trees before build_counts/set_counts");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, mvhdp_launch_build_trees(h->mm, false, true, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.trees_built(true, false);
    return MVHDP_OK;
}

extern "C" int mvhdp_build_inference_trees(mvhdp_handle h)
{
    CHECK_H(h);
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "build_inference_trees before set_hyper");
    if (!h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "build_inference_trees before build_counts/set_counts");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, mvhdp_launch_build_trees(h->mm, true, true, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.trees_built(true, true);
    return MVHDP_OK;
}

extern "C" int mvhdp_init_assignments_from_trees(mvhdp_handle h, uint64_t seed)
{
    CHECK_H(h);
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->st.trees_current()) FAIL(h, MVHDP_ERR_STATE, "init_assignments_from_trees before build_trees/build_inference_trees");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, mvhdp_launch_init_from_trees(h->mm, (uint32_t)seed, (uint32_t)(seed >> 32), h->stream));     // reads the descent table only
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.assignments_replaced(-1, false);                                                                   // (every token got a topic, INF:169-199)
    return MVHDP_OK;
}

extern "C" int mvhdp_get_counts(mvhdp_handle h, int32_t m, int32_t* n_wk, int32_t* n_k)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_counts: bad view");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    const int K = mm.K;
    if (n_wk) HIPC(h, hipMemcpy(n_wk, mm.counts + mm.rowbase[m] * K, (size_t)mm.V[m] * K * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_k) HIPC(h, hipMemcpy(n_k, mm.counts + mm.rowbase[mm.M] * K + (int64_t)m * K, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_set_counts(mvhdp_handle h, int32_t m, const int32_t* n_wk, const int32_t* n_k)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_counts: bad view");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    const int K = mm.K;
    if (n_wk) HIPC(h, hipMemcpy(mm.counts + mm.rowbase[m] * K, n_wk, (size_t)mm.V[m] * K * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_k) HIPC(h, hipMemcpy(mm.counts + mm.rowbase[mm.M] * K + (int64_t)m * K, n_k, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice));
    h->st.counts_rebuilt();
    return MVHDP_OK;
}

extern "C" int mvhdp_get_tree(mvhdp_handle h, int32_t m, int32_t type, double* tree)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M || type < 0 || type >= mm.V[m] || !tree) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_tree: bad argument");
    if (!h->st.trees_current()) FAIL(h, MVHDP_ERR_STATE, "get_tree before build_trees");
    HIPC(h, hipSetDevice(h->device));
    { int rc2 = ensure_full_trees(h); if (rc2) return rc2; }
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipMemcpy(tree, mm.trees + (mm.rowbase[m] + type) * 2 * mm.K, (size_t)2 * mm.K * sizeof(double), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_get_doc_topic_hist(mvhdp_handle h, int32_t m, int32_t* hist, int32_t hist_len,
                                        int32_t* doc_len_counts, int32_t len_len)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M || (hist && hist_len < 1) || (doc_len_counts && len_len < 1))
        FAIL(h, MVHDP_ERR_INVALID_ARG, "get_doc_topic_hist: bad argument");
    int rc = require_corpus(h); if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    DevArray<int32_t> d_hist, d_len;
    if (hist) HIPC(h, d_hist.alloc((size_t)mm.K * hist_len));
    if (doc_len_counts) HIPC(h, d_len.alloc((size_t)len_len));
    HIPC(h, mvhdp_launch_doc_topic_hist(mm, m, d_hist, hist_len, d_len, len_len, h->stream));   // (waits for the stream)
    if (hist) HIPC(h, hipMemcpy(hist, d_hist, d_hist.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (doc_len_counts) HIPC(h, hipMemcpy(doc_len_counts, d_len, d_len.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

// Largest entity (sizes the slot list) and the work-queue order: longest entities first,
// so that the tail of the sweep is made of short ones (power-law lengths).
int64_t compute_max_doc_tokens(mvhdp_ctx* h)
{
    if (h->max_doc_tokens >= 0) return h->max_doc_tokens;
    int64_t mx = 0, mn = INT64_MAX;
    const MvModel& mm = h->mm;
    std::vector<int64_t> tot((size_t)mm.D);
    for (int64_t d = 0; d < mm.D; d++) {
        int64_t t = 0;
        for (int m = 0; m < mm.M; m++) t += h->h_doc_off[m][d + 1] - h->h_doc_off[m][d];
        tot[d] = t;
        mx = std::max(mx, t); mn = std::min(mn, t);
    }
    if (h->d_doc_order) { hipFree(h->d_doc_order); h->d_doc_order = nullptr; }
    h->tokens_desc.clear();
    if (mm.D > 0 && mm.D < (1LL << 31)) {
        // counting sort by decreasing length (stable: ties keep entity order)
        std::vector<int64_t> start((size_t)mx + 2, 0);
        for (int64_t d = 0; d < mm.D; d++) start[(size_t)(mx - tot[d]) + 1]++;
        for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
        std::vector<int32_t> order((size_t)mm.D);
        for (int64_t d = 0; d < mm.D; d++) order[(size_t)start[(size_t)(mx - tot[d])]++] = (int32_t)d;
        // without the order on the device the sweep runs in natural entity order (correct, only less balanced)
        if (hipMalloc(&h->d_doc_order, (size_t)mm.D * sizeof(int32_t)) != hipSuccess) h->d_doc_order = nullptr;
        else if (hipMemcpy(h->d_doc_order, order.data(), (size_t)mm.D * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(h->d_doc_order); h->d_doc_order = nullptr;
        } else {
            h->tokens_desc.resize((size_t)mm.D);
            for (int64_t q = 0; q < mm.D; q++) h->tokens_desc[(size_t)q] = tot[(size_t)order[(size_t)q]];
        }
    }
    (void)mn;
    h->max_doc_tokens = mx;
    return mx;
}

// UPD:263-270: the topic leaves inActiveTopicIndex and its alpha[m][k] takes alpha[m][K]
int apply_activation(mvhdp_ctx* h, int32_t activated_topic, int32_t activated_modality)
{
    MvModel& mm = h->mm;
    if (activated_topic < 0) return MVHDP_OK;
    if (activated_topic >= mm.K || activated_modality < 0 || activated_modality >= mm.M)
        FAIL(h, MVHDP_ERR_INVALID_ARG, "apply_delta: bad activation");
    if (h->h_inactive[activated_topic]) {
        h->h_inactive[activated_topic] = 0;
        h->h_alpha[(size_t)activated_modality * (mm.K + 1) + activated_topic] = h->h_alpha[(size_t)activated_modality * (mm.K + 1) + mm.K];
        mm.first_inactive = -1;
        for (int k = 0; k < mm.K; k++) if (h->h_inactive[k]) { mm.first_inactive = k; break; }
        HIPC(h, hipMemcpy(h->d_alpha, h->h_alpha.data(), h->h_alpha.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPC(h, hipMemcpy(h->d_inactive, h->h_inactive.data(), (size_t)mm.K, hipMemcpyHostToDevice));
    }
    return MVHDP_OK;
}

// MVHDP_BUF_BIRTH_KEYS after a NO_APPLY sweep of a document shard, MIN-reduced over the shards: every replica activates the same
// topics.  The table is checked whole before anything changes (see include/mvhdp.h).
int mvhdp_activate_births_ex(mvhdp_ctx* h, const int64_t* keys, int* n_born, long long* first_key)
{
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (n_born) *n_born = 0;
    if (first_key) *first_key = LLONG_MAX;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "activate_births before set_hyper");
    if (h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "activate_births inside an mvhdp_apply_delta_begin bracket (call mvhdp_apply_delta_end first)");
    if (h->st.delta_pending()) FAIL(h, MVHDP_ERR_STATE, "activate_births: the NO_APPLY sweep's deltas have not been applied (mvhdp_apply_delta first)");
    std::vector<long long> tab((size_t)K);
    HIPC(h, hipSetDevice(h->device));
    if (keys) std::copy(keys, keys + K, tab.begin());
    else {
        HIPC(h, hipMemcpyAsync(tab.data(), h->d_birth_table, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    std::vector<std::pair<int32_t, long long>> born;
    for (int k = 0; k < K; k++) {
        const long long key = tab[(size_t)k];
        if (key == LLONG_MAX) continue;
        if (key < 0 || MVHDP_ACT_KEY_TOPIC(key) != k) FAIL(h, MVHDP_ERR_INVALID_ARG, "activate_births: a key's topic field is not its index");
        if (MVHDP_ACT_KEY_VIEW(key) >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "activate_births: a key's view is beyond the model's views");
        if (!h->h_inactive[k]) FAIL(h, MVHDP_ERR_INVALID_ARG, "activate_births: a key on a topic that is already active");
        born.emplace_back(k, key);
    }
    // every shard moves forward along the same list of inactive topics: what any of them reached is a prefix of it
    size_t i = 0;
    for (int k = 0; k < K && i < born.size(); k++)
        if (h->h_inactive[k]) { if (born[i].first != k) FAIL(h, MVHDP_ERR_INVALID_ARG, "activate_births: the births are not a prefix of the inactive topics"); i++; }
    SweepOutcome oc;
    const int rc = activate_born(h, born, oc);
    if (rc) return rc;
    if (n_born) *n_born = oc.n_activations;
    if (first_key) *first_key = oc.first_act;
    return MVHDP_OK;
}

extern "C" int mvhdp_activate_births(mvhdp_handle h, const int64_t* keys)
{
    CHECK_H(h);
    return mvhdp_activate_births_ex(h, keys, nullptr, nullptr);
}

extern "C" int mvhdp_get_birth_keys(mvhdp_handle h, int64_t* keys)
{
    CHECK_H(h);
    if (!keys) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_birth_keys: null");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(keys, h->d_birth_table, (size_t)h->mm.K * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

extern "C" int mvhdp_apply_delta(mvhdp_handle h, int32_t activated_topic, int32_t activated_modality)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemsetAsync(h->d_stats + ST_NEGATIVE, 0, sizeof(unsigned long long), h->stream));
    HIPC(h, mvhdp_launch_apply_delta(mm, h->d_stats, h->stream, h->st.delta16_used()));
    h->st.delta16_rebiased();
    unsigned long long neg = 0;
    HIPC(h, hipMemcpyAsync(&neg, h->d_stats + ST_NEGATIVE, sizeof neg, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.delta_applied();                                       // apply_delta_kernel zeroes what it adds
    { int rc = apply_activation(h, activated_topic, activated_modality); if (rc) return rc; }
    if (neg) FAIL(h, MVHDP_ERR_NEGATIVE_COUNT, "a topic count went below zero (UPD:202-215)");
    return MVHDP_OK;
}

// ---- the multi-GPU pipeline: apply + tree rebuild by row ranges, stream-ordered (see include/mvhdp.h) ----
extern "C" int mvhdp_apply_delta_begin(mvhdp_handle h)
{
    CHECK_H(h);
    if (!h->have_hyper || !h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "apply_delta_begin before set_hyper / counts");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemsetAsync(h->d_stats + ST_NEGATIVE, 0, sizeof(unsigned long long), h->stream));
    HIPC(h, mvhdp_launch_apply_nk(h->mm, h->d_stats + ST_NEGATIVE, h->stream));
    h->st.bracket_begun();
    return MVHDP_OK;
}

extern "C" int mvhdp_apply_delta_rows(mvhdp_handle h, int64_t row_begin, int64_t row_end)
{
    CHECK_H(h);
    const int64_t nrows = h->mm.rowbase[h->mm.M];
    if (!h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "apply_delta_rows outside an apply_delta_begin / apply_delta_end bracket");
    if (row_begin < 0 || row_end > nrows || row_begin > row_end) FAIL(h, MVHDP_ERR_INVALID_ARG, "apply_delta_rows: bad row range");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, mvhdp_launch_build_trees_rows(h->mm, false, h->st.last_need_full(), row_begin, row_end, true, h->d_stats + ST_NEGATIVE, h->stream));
    h->st.bracket_rows(row_end - row_begin);
    return MVHDP_OK;
}

extern "C" int mvhdp_apply_delta_end(mvhdp_handle h, int32_t activated_topic, int32_t activated_modality)
{
    CHECK_H(h);
    const int64_t nrows = h->mm.rowbase[h->mm.M];
    if (!h->st.bracket_closed(nrows)) FAIL(h, MVHDP_ERR_STATE, "apply_delta_end: the row ranges applied do not cover every row exactly once");
    HIPC(h, hipSetDevice(h->device));
    unsigned long long neg = 0;
    HIPC(h, hipMemcpyAsync(&neg, h->d_stats + ST_NEGATIVE, sizeof neg, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->st.delta_zeroed();
    // the trees were rebuilt from the updated counts row by row: current, unless an activation now changes alpha
    h->st.trees_built(h->st.last_need_full(), false);
    if (activated_topic >= 0) {
        h->st.trees_outdated();
        int rc = apply_activation(h, activated_topic, activated_modality);
        if (rc) return rc;
    }
    if (neg) FAIL(h, MVHDP_ERR_NEGATIVE_COUNT, "a topic count went below zero (UPD:202-215)");
    return MVHDP_OK;
}

extern "C" int mvhdp_trees_current(mvhdp_handle h)
{
    CHECK_H(h);
    return h->st.trees_current() ? 1 : 0;
}

// ---- tuning: what a host may pin, what the library has learnt (so that a document shard, a resumed chain or another handle on
// the same corpus does not search again) ----
extern "C" int mvhdp_get_tuning(mvhdp_handle h, mvhdp_tuning* t)
{
    CHECK_H(h);
    if (!t) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_tuning: null");
    memset(t, 0, sizeof *t);
    t->force_primary = h->tu.force_primary; t->narrow = h->tu.narrow; t->walk_fixed = h->tu.walk_fixed;
    t->single_stream = h->tu.single_stream; t->primary_min_share = h->tu.primary_min_share; t->live16 = h->tu.live16;
    t->single_wave = h->tu.single_wave; t->live_overlap = h->tu.live_overlap; t->live_rows = h->tu.live_rows;
    for (int m = 0; m < MVHDP_MAX_MODALITIES; m++) { t->walk_theta[m] = h->tu.walk_theta[m]; t->tree_branch_share[m] = h->wt.walk_f[m]; }
    for (int g = 0; g < WALK_GROUPS; g++) t->learnt_walk_step[g] = g == h->wt.walk_cls ? h->wt.walk_i : h->wt.walk_i_by[g];
    t->learnt_walk_step[3] = -1;
    return MVHDP_OK;
}

extern "C" int mvhdp_set_tuning(mvhdp_handle h, const mvhdp_tuning* t)
{
    CHECK_H(h);
    if (!t) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_tuning: null");
    const int fp = t->force_primary;
    if (!(fp == 0 || fp == 1 || fp == 2 || fp == 4 || fp == 8 || fp == 16 || fp == 32)) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_tuning: force_primary must be 0, 1, 2, 4, 8, 16 or 32");
    if (t->primary_min_share < 0.0 || t->primary_min_share > 1.0) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_tuning: primary_min_share outside [0, 1]");
    for (int g = 0; g < WALK_GROUPS; g++) if (t->learnt_walk_step[g] < -1 || t->learnt_walk_step[g] > MVHDP_WALK_BINS) FAIL(h, MVHDP_ERR_INVALID_ARG, "set_tuning: learnt_walk_step outside [-1, 20]");
    h->tu.force_primary = fp; h->tu.narrow = t->narrow; h->tu.walk_fixed = t->walk_fixed ? 1 : 0;
    h->tu.single_stream = t->single_stream ? 1 : 0;
    h->tu.live16 = t->live16 < 0 ? -1 : (t->live16 ? 1 : 0);
    h->tu.single_wave = t->single_wave ? 1 : 0;
    h->tu.live_overlap = t->live_overlap < 0 ? -1 : (t->live_overlap ? 1 : 0);
    h->tu.live_rows = t->live_rows < 0 ? -1 : (t->live_rows ? 1 : 0);
    h->tu.primary_min_share = t->primary_min_share > 0.0 ? t->primary_min_share : 0.10;
    for (int m = 0; m < MVHDP_MAX_MODALITIES; m++) h->tu.walk_theta[m] = t->walk_theta[m];
    if (t->learnt_walk_step[0] >= 0 || t->learnt_walk_step[1] >= 0 || t->learnt_walk_step[2] >= 0) h->wt.restore(t->learnt_walk_step, t->tree_branch_share, h->mm.M);
    return MVHDP_OK;
}

// The planner and the walk search without a device (tests/test_plan.py): pure functions of their arguments.
extern "C" int mvhdp_plan_probe(const mvhdp_plan_input* pi, const mvhdp_tuning* t, mvhdp_plan_output* po)
{
    if (!pi || !po) return MVHDP_ERR_INVALID_ARG;
    PlanIn in;
    in.K = pi->num_topics; in.M = pi->num_modalities; in.D = pi->num_entities; in.mdt = pi->max_entity_tokens;
    if (in.K < 1 || in.K > MVHDP_MAX_TOPICS || in.M < 1 || in.M > MVHDP_MAX_MODALITIES || in.D < 0) return MVHDP_ERR_INVALID_ARG;
    in.have_order = true;
    for (int c = 0; c < 5; c++) in.n_longer[c] = pi->entities_longer_than[c];
    for (int b = 0; b < MVHDP_HIST_BINS; b++) in.tok_hist[b] = pi->tokens_by_list_rounds[b];
    for (int b = 0; b < MVHDP_ENT_BINS; b++) in.ent_hist[b] = pi->entities_by_class[b];
    in.flags = pi->flags; in.debug = pi->debug != 0; in.batch = pi->batch != 0; in.trees_current = pi->trees_current != 0;
    in.first_inactive = pi->inactive_topics ? 0 : -1;
    in.unassigned = pi->unassigned != 0;
    in.num_cus = pi->num_cus > 0 ? pi->num_cus : 256;
    for (int c = 0; c < MVHDP_N_CLASSES; c++) for (int f = 0; f < 3; f++) in.regs.regs[c][f] = pi->kernel_registers[c][f];
    // (a probe that names no register counts for the mix flavours sizes them as the plain ones)
    for (int c = 0; c < MVHDP_N_CLASSES; c++) for (int f = 0; f < 3; f++) in.regs.regs_mix[c][f] = pi->kernel_registers_mix[c][f] > 0 ? pi->kernel_registers_mix[c][f] : pi->kernel_registers[c][f];
    in.vectors_mix = pi->vectors_mix != 0 && !(pi->flags & MVHDP_SWEEP_FROZEN);
    in.slim_table = t && t->narrow == 2;                  // (a probe whose tuning says narrow = 2: a handle that keeps the 12-bit image; views below 2^28 types)
    PlanTuning tu;
    WalkTuner wt;
    wt.init_defaults(in.K);
    if (t) {
        tu.force_primary = t->force_primary; tu.narrow = t->narrow; tu.walk_fixed = t->walk_fixed; tu.single_stream = t->single_stream;
        tu.live16 = t->live16; tu.single_wave = t->single_wave ? 1 : 0; tu.live_overlap = t->live_overlap; tu.live_rows = t->live_rows;
        if (t->primary_min_share > 0) tu.primary_min_share = t->primary_min_share;
        for (int m = 0; m < MVHDP_MAX_MODALITIES; m++) tu.walk_theta[m] = t->walk_theta[m];
        if (t->learnt_walk_step[0] >= 0 || t->learnt_walk_step[1] >= 0 || t->learnt_walk_step[2] >= 0) wt.restore(t->learnt_walk_step, t->tree_branch_share, in.M);
    }
    SweepPlan p;
    plan_sweep(in, tu, wt, p);
    memset(po, 0, sizeof *po);
    po->status = p.err;
    if (p.err) return MVHDP_OK;
    po->segments = p.nseg; po->primary_class = p.pc; po->routed_prefix = p.H; po->register_resident = p.fast ? 1 : 0;
    po->need_full_trees = p.need_full ? 1 : 0; po->dominant_class = p.dominant;
    for (int c = 0; c < MVHDP_N_CLASSES; c++) {
        po->class_used[c] = p.cls[c].used ? 1 : 0; po->class_map[c] = p.class_map[c];
        po->class_stream[c] = p.cls[c].stream; po->class_grid[c] = p.cls[c].grid; po->class_lds_bytes[c] = (int64_t)p.cls[c].lds;
        po->class_walk[c] = p.cls[c].walk; po->class_narrow[c] = p.cls[c].narrow; po->class_register_resident[c] = p.cls[c].fast ? 1 : 0;
        po->class_theta0[c] = p.cls[c].theta[0];
    }
    po->delta16 = p.delta16 ? 1 : 0;
    po->live_rows = p.live_rows ? 1 : 0;
    return MVHDP_OK;
}

extern "C" int mvhdp_tuner_probe(int32_t num_modalities, const double* tree_branch_share, const double* u1_hist, const double* ns_by_step /*[21]*/,
                                 int32_t n_sweeps, int32_t group, int32_t* steps_out /*[n_sweeps]*/)
{
    if (!tree_branch_share || !ns_by_step || !steps_out || num_modalities < 1 || num_modalities > MVHDP_MAX_MODALITIES || n_sweeps < 0) return MVHDP_ERR_INVALID_ARG;
    WalkTuner wt;
    if (group < 0 || group >= WALK_GROUPS) return MVHDP_ERR_INVALID_ARG;
    for (int m = 0; m < num_modalities; m++) wt.walk_f[m] = tree_branch_share[m];
    for (int b = 0; b < MVHDP_WALK_BINS; b++) wt.walk_hist[b] = u1_hist ? u1_hist[b] : 0.0;
    for (int i = 0; i < n_sweeps; i++) {
        double theta[WALK_GROUPS][MVHDP_MAXM]; bool measure;
        wt.propose(group, num_modalities, theta, &measure);
        steps_out[i] = wt.walk_probe_i;
        wt.observe(true, 1, num_modalities, ns_by_step[std::max(0, std::min(MVHDP_WALK_BINS, wt.walk_probe_i))]);
    }
    return MVHDP_OK;
}

extern "C" int mvhdp_get_view_weights(mvhdp_handle h, double* p)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (!p) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_view_weights: null");
    if (mm.M == 1) { for (int64_t d = 0; d < mm.D; d++) p[d] = 1.0; return MVHDP_OK; }
    if (!mm.p) FAIL(h, MVHDP_ERR_STATE, "get_view_weights before the first sweep");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipMemcpy(p, mm.p, (size_t)mm.D * mm.M * mm.M * sizeof(double), hipMemcpyDeviceToHost));
    return MVHDP_OK;
}

extern "C" int mvhdp_device_buffer(mvhdp_handle h, mvhdp_buffer which, void** dev_ptr, size_t* bytes)
{
    CHECK_H(h);
    if (!dev_ptr || !bytes) FAIL(h, MVHDP_ERR_INVALID_ARG, "device_buffer: null");
    size_t b = (size_t)counts_len(h) * sizeof(int32_t);
    if (which == MVHDP_BUF_COUNTS) { *dev_ptr = h->mm.counts; *bytes = b; return MVHDP_OK; }
    if (which == MVHDP_BUF_DELTA) { *dev_ptr = h->mm.delta; *bytes = b; return MVHDP_OK; }
    if (which == MVHDP_BUF_BIRTH_KEYS) { *dev_ptr = h->d_birth_table; *bytes = (size_t)h->mm.K * sizeof(long long); return MVHDP_OK; }
    if (which == MVHDP_BUF_COUNTS12 && h->mm.counts12) { *dev_ptr = h->mm.counts12; *bytes = (size_t)h->mm.rowbase[h->mm.M] * mvhdp_slim_row_bytes(h->mm.K); return MVHDP_OK; }
    if (which == MVHDP_BUF_ROW_CLASS) { *dev_ptr = h->mm.heavy; *bytes = (size_t)h->mm.rowbase[h->mm.M]; return MVHDP_OK; }
    FAIL(h, MVHDP_ERR_INVALID_ARG, "device_buffer: unknown buffer (or a handle without that table)");
}

extern "C" int mvhdp_counts_written(mvhdp_handle h)
{
    CHECK_H(h);
    h->st.counts_rebuilt();
    return MVHDP_OK;
}

// ---------------------------------------------------------------------------
// statistics for optimizeBeta / optimizeP and the log likelihood
// ---------------------------------------------------------------------------
// MALLET 2.0.8 Dirichlet.logGammaStirling (restated from the class file's bytecode)
static double log_gamma_stirling_host(double z)
{
    const double HALF_LOG_TWO_PI = std::log(6.283185307179586) / 2.0;
    int shift = 0;
    while (z < 2.0) { z = z + 1; shift++; }
    double result = HALF_LOG_TWO_PI + (z - 0.5) * std::log(z) - z + 1 / (12.0 * z) - 1 / (360.0 * z * z * z)
                    + 1 / (1260.0 * z * z * z * z * z);
    while (shift > 0) { shift--; z = z - 1; result = result - std::log(z); }
    return result;
}

extern "C" int mvhdp_get_count_histogram(mvhdp_handle h, int32_t m, int32_t* hist, int32_t len)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M || !hist || len < 1) FAIL(h, MVHDP_ERR_INVALID_ARG, "get_count_histogram: bad argument");
    if (!h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "get_count_histogram before build_counts/set_counts");
    HIPC(h, hipSetDevice(h->device));
    DevArray<int32_t> d;
    HIPC(h, d.alloc((size_t)len));
    HIPC(h, mvhdp_launch_count_hist(mm, m, d, len, h->stream));
    HIPC(h, d.download(hist, (size_t)len, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

// optimizeP PTM:2706-2792: acc[m*M+i] += pDistr_Mean[m][i][doc] over this handle's entities, one after the other in entity order
// (PTM:2789-2792).  A group of document shards in ONE process hands the accumulators from member to member (ascending doc_id_base): the
// additions are then the single handle's, in the same order, bit for bit.
int mvhdp_view_overlap_accumulate(mvhdp_ctx* h, double* acc)
{
    MvModel& mm = h->mm;
    int rc = require_corpus(h); if (rc) return rc;
    const int M = mm.M;
    if (mm.D == 0) return MVHDP_OK;
    HIPC(h, hipSetDevice(h->device));
    DevArray<double> d;
    const size_t n = (size_t)M * M * mm.D;
    HIPC(h, d.alloc(n));
    std::vector<double> host(n);
    HIPC(h, mvhdp_launch_view_overlap(mm, d, h->stream));
    HIPC(h, d.download(host.data(), n, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < M * M; i++) {                     // PTM:2789-2792: sequential, entity order
        double a = acc[i];
        const double* col = host.data() + (size_t)i * mm.D;
        for (int64_t doc = 0; doc < mm.D; doc++) a += col[doc];
        acc[i] = a;
    }
    return MVHDP_OK;
}

extern "C" int mvhdp_view_overlap_sums(mvhdp_handle h, double* sums)
{
    CHECK_H(h);
    if (!sums) FAIL(h, MVHDP_ERR_INVALID_ARG, "view_overlap_sums: null");
    for (int i = 0; i < h->mm.M * h->mm.M; i++) sums[i] = 0.0;
    return mvhdp_view_overlap_accumulate(h, sums);
}

// What the proportions need before their kernel runs: every view's corpus, the hyper-parameters, and per view the carry-over map of
// PTM:2873-2886 (built once per corpus).  Shared with the thresholded lists and entity distributions of mvhdp_sim.hip.
int mvhdp_doc_topic_prepare(mvhdp_ctx* h, DocTopicCarry& carry)
{
    MvModel& mm = h->mm;
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "doc_topic_proportions before set_hyper");
    HIPC(h, hipSetDevice(h->device));
    for (int m = 0; m < mm.M; m++) {
        if (!h->d_carry[m] && mm.D > 0) {                  // PTM:2873-2886: a missing view keeps the previous entity's counts
            std::vector<int64_t> src((size_t)mm.D);
            int64_t last = -1;
            for (int64_t d = 0; d < mm.D; d++) {
                const bool has = h->h_present[m].empty() ? h->h_doc_off[m][d + 1] > h->h_doc_off[m][d] : h->h_present[m][(size_t)d] != 0;
                if (has) last = d;                             // (a present view without tokens is refreshed to zeros, PTM:2873-2886)
                src[(size_t)d] = last;
            }
            DevArray<int64_t> d_src;                           // the handle's only once it is filled
            HIPC(h, d_src.alloc(src.size()));
            HIPC(h, hipMemcpy(d_src, src.data(), src.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            h->d_carry[m] = d_src.release();
        }
        carry.src[m] = h->d_carry[m];
    }
    return MVHDP_OK;
}

extern "C" int mvhdp_doc_topic_proportions(mvhdp_handle h, const double* view_weights, int64_t d0, int64_t d1, double* out)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "doc_topic_proportions before set_hyper");
    if (!view_weights || !out || d0 < 0 || d1 > mm.D || d0 > d1) FAIL(h, MVHDP_ERR_INVALID_ARG, "doc_topic_proportions: bad range or null buffer");
    if (d1 == d0) return MVHDP_OK;
    DocTopicCarry carry{};
    rc = mvhdp_doc_topic_prepare(h, carry); if (rc) return rc;
    DevArray<double> d_w, d_out;
    const size_t n = (size_t)(d1 - d0) * mm.K;
    HIPC(h, d_w.alloc((size_t)mm.M));
    HIPC(h, d_out.alloc(n));
    HIPC(h, d_w.upload(view_weights, (size_t)mm.M, h->stream));
    HIPC(h, mvhdp_launch_doc_topic_prop(mm, carry, d_w, d0, d1, d_out, h->stream));
    HIPC(h, d_out.download(out, n, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

extern "C" int mvhdp_gamma_doc_statistics(mvhdp_handle h, int32_t m, double gamma_m, uint64_t seed, uint32_t round, double* qs, double* qw)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    if (m < 0 || m >= mm.M || !qs || !qw || !(gamma_m > 0.0)) FAIL(h, MVHDP_ERR_INVALID_ARG, "gamma_doc_statistics: bad argument");
    int rc = require_corpus(h); if (rc) return rc;
    *qs = 0; *qw = 0;
    if (mm.D == 0) return MVHDP_OK;
    HIPC(h, hipSetDevice(h->device));
    const int NB = 1024;                                   // fixed: the summation order is part of the result
    DevArray<double> d_part;
    std::vector<double> part(2 * NB);
    HIPC(h, d_part.alloc(2 * NB));
    HIPC(h, mvhdp_launch_gamma_doc_stats(mm, m, gamma_m, (uint32_t)seed, (uint32_t)(seed >> 32), round, d_part, NB, h->stream));
    HIPC(h, d_part.download(part.data(), 2 * NB, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    double a = 0, b = 0;
    for (int i = 0; i < NB; i++) { a += part[2 * i]; b += part[2 * i + 1]; }
    *qs = a; *qw = b;
    return MVHDP_OK;
}

// optimizeDP's view-table simulation PTM:2454-2488 on the device (opt-in: mvhdp_stats.hip dp_tables_kernel).  The histogram comes from
// the host -- a single handle's mvhdp_get_doc_topic_hist or a sharded model's mvhdp_group_doc_topic_hist: the draw of a cell belongs to
// the WHOLE model's cell, so the statistic is the same however the entities are sharded.
extern "C" int mvhdp_dp_table_statistics(mvhdp_handle h, int32_t m, const int32_t* hist, int32_t hist_len, const double* conc, uint64_t seed, uint32_t round,
                                         double* mk, uint8_t* active)
{
    CHECK_H(h);
    MvModel& mm = h->mm;
    const int K = mm.K;
    if (m < 0 || m >= mm.M || !hist || hist_len < 1 || !conc || !mk || !active) FAIL(h, MVHDP_ERR_INVALID_ARG, "dp_table_statistics: bad argument");
    HIPC(h, hipSetDevice(h->device));
    const size_t hb = (size_t)K * hist_len * sizeof(int32_t);
    DevArray<char> d;                                      // one block: hist [K][hist_len], padded to 8 bytes | conc [K] | mk [K] | active [K]
    HIPC(h, d.alloc(hb + (size_t)K * (2 * sizeof(double) + 8)));
    int32_t* d_hist = (int32_t*)d.get();
    double* d_conc = (double*)(d.get() + ((hb + 7) & ~(size_t)7));
    double* d_mk = d_conc + K;
    uint8_t* d_act = (uint8_t*)(d_mk + K);
    HIPC(h, hipMemcpyAsync(d_hist, hist, hb, hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(d_conc, conc, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, mvhdp_launch_dp_tables(d_hist, hist_len, K, m, d_conc, (uint32_t)seed, (uint32_t)(seed >> 32), round, d_mk, d_act, h->stream));
    HIPC(h, hipMemcpyAsync(mk, d_mk, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(active, d_act, (size_t)K, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

// n independent Antoniak draws (optimizeDP's root level PTM:2491-2517 with the device option): see antoniak_draws_kernel
extern "C" int mvhdp_antoniak_draws(mvhdp_handle h, int32_t n, const int32_t* items, const double* conc, uint64_t seed, uint32_t round, int32_t* tables)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!items || !conc || !tables))) FAIL(h, MVHDP_ERR_INVALID_ARG, "antoniak_draws: bad argument");
    if (n == 0) return MVHDP_OK;
    HIPC(h, hipSetDevice(h->device));
    DevArray<char> d;                                      // one block: conc [n] | items [n] | tables [n]
    HIPC(h, d.alloc((size_t)n * (sizeof(double) + 2 * sizeof(int32_t))));
    double* d_conc = (double*)d.get(); int32_t* d_items = (int32_t*)(d_conc + n); int32_t* d_tab = d_items + n;
    HIPC(h, hipMemcpyAsync(d_conc, conc, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(d_items, items, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, mvhdp_launch_antoniak_draws(n, d_items, d_conc, (uint32_t)seed, (uint32_t)(seed >> 32), round, d_tab, h->stream));
    HIPC(h, hipMemcpyAsync(tables, d_tab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return MVHDP_OK;
}

// modelLogLikelihood PTM:3322-3452 in two parts, so that a group of document shards can put them together (mvhdp_group_log_likelihood):
// the DOCUMENT part of view m (PTM:3341-3367) belongs to the entities of a handle -- *ll and *cnt (modalityCnt) continue a sequential
// sum in entity order --, the MODEL part (PTM:3373-3441: the modalityCnt term, the topic-word term over n_wk, the n_k terms) to the
// replicated counts: once per model.
int mvhdp_ll_doc_accumulate(mvhdp_ctx* h, int m, double* ll, int64_t* cnt)
{
    MvModel& mm = h->mm;
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "model_log_likelihood before set_hyper");
    if (m < 0 || m >= mm.M) FAIL(h, MVHDP_ERR_INVALID_ARG, "model_log_likelihood: bad view");
    if (mm.D == 0) return MVHDP_OK;
    HIPC(h, hipSetDevice(h->device));
    DevArray<double> d_doc;
    HIPC(h, d_doc.alloc((size_t)mm.D));
    std::vector<double> hdoc((size_t)mm.D);
    HIPC(h, mvhdp_launch_loglik_doc(mm, m, d_doc, h->stream));
    HIPC(h, d_doc.download(hdoc.data(), (size_t)mm.D, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    double a = *ll;
    int64_t c = *cnt;
    for (int64_t d = 0; d < mm.D; d++) {
        const bool has = h->h_present[m].empty() ? h->h_doc_off[m][d + 1] > h->h_doc_off[m][d] : h->h_present[m][(size_t)d] != 0;
        if (has) { a += hdoc[d]; c++; }                                                              // PTM:3348-3367
    }
    *ll = a; *cnt = c;
    return MVHDP_OK;
}

int mvhdp_ll_model_finish(mvhdp_ctx* h, int m, double ll, int64_t modalityCnt, double* out)
{
    MvModel& mm = h->mm;
    if (!h->have_hyper || !h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "model_log_likelihood before set_hyper/build_counts");
    if (m < 0 || m >= mm.M || !out) FAIL(h, MVHDP_ERR_INVALID_ARG, "model_log_likelihood: bad view");
    const int M = mm.M, K = mm.K;
    ll += modalityCnt * log_gamma_stirling_host((double)mm.gamma[m] * mm.alpha_sum[m]);           // PTM:3373
    if (std::isnan(ll) || std::isinf(ll)) { *out = 0; return MVHDP_OK; }                           // PTM:3375-3383
    HIPC(h, hipSetDevice(h->device));
    const int NP = 1024;
    DevArray<double> d_part;
    DevArray<unsigned long long> d_nz;
    HIPC(h, d_part.alloc(NP));
    HIPC(h, d_nz.alloc(1));
    std::vector<double> hpart(NP);
    std::vector<int32_t> nk((size_t)K);
    unsigned long long nz = 0;
    HIPC(h, mvhdp_launch_loglik_topic(mm, m, d_part, NP, d_nz, h->stream));
    HIPC(h, d_part.download(hpart.data(), NP, h->stream));
    HIPC(h, d_nz.download(&nz, 1, h->stream));
    HIPC(h, hipMemcpyAsync(nk.data(), mm.counts + mm.rowbase[M] * K + (int64_t)m * K, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < NP; i++) ll += hpart[i];                                                    // PTM:3389-3415
    if (std::isnan(ll) || std::isinf(ll)) ll = 0;
    const double bv = mm.beta[m] * mm.V[m];
    for (int topic = 0; topic < K; topic++) {                                                       // PTM:3417-3435
        ll -= (bv + nk[topic]) == 0 ? 0 : log_gamma_stirling_host(bv + nk[topic]);
        if (std::isnan(ll) || std::isinf(ll)) ll = 0;
    }
    ll += bv == 0 ? 0 : log_gamma_stirling_host(bv) * K;                                            // PTM:3438
    ll -= mm.beta[m] == 0 ? 0 : log_gamma_stirling_host(mm.beta[m]) * (double)nz;                   // PTM:3441
    if (std::isinf(ll)) ll = 0;
    *out = ll;
    return MVHDP_OK;
}

extern "C" int mvhdp_model_log_likelihood(mvhdp_handle h, double* out)
{
    CHECK_H(h);
    if (!out) FAIL(h, MVHDP_ERR_INVALID_ARG, "model_log_likelihood: null");
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper || !h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "model_log_likelihood before set_hyper/build_counts");
    for (int m = 0; m < h->mm.M; m++) {
        double ll = 0;
        int64_t cnt = 0;
        rc = mvhdp_ll_doc_accumulate(h, m, &ll, &cnt); if (rc) return rc;
        rc = mvhdp_ll_model_finish(h, m, ll, cnt, &out[m]); if (rc) return rc;
    }
    return MVHDP_OK;
}
