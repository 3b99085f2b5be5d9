// mvhdp_enqueue.hip — the sweep of one handle: plan (mvhdp_plan.h) -> enqueue -> finish, and the entry points built on it
// (mvhdp_sweep, mvhdp_sweep_many; mvhdp_sweep_begin / mvhdp_sweep_finish for a group of document shards).
#include "mvhdp_ctx.h"

// Births of a live sweep, chunk by chunk (SweepLaunch::births): the reference's updater takes a topic out of inActiveTopicIndex with the
// FIRST delta that reaches it (UPD:263-270) and its samplers then draw the next inactive index (WRK:523-526) -- all 100 inactive topics of
// C5 are active within its first sweep.  A segment starts with the list of the topics that are inactive now (births_begin); its kernels
// move along that list as their chunks' deltas land; births_end activates what was reached, in index order, each topic's alpha[m][K]
// going to the view of its first delta.
static hipError_t births_begin(mvhdp_ctx* h, hipStream_t s)
{
    const int K = h->mm.K;
    h->h_births.assign((size_t)2 + 2 * K, -1);
    int n = 0;
    for (int k = 0; k < K; k++) if (h->h_inactive[k]) { h->h_births[(size_t)2 + K + k] = n; h->h_births[(size_t)2 + n++] = k; }
    h->h_births[0] = 0; h->h_births[1] = n;
    h->h_birth_keys.assign((size_t)K, LLONG_MAX);
    hipError_t e = hipMemcpyAsync(h->d_births, h->h_births.data(), h->h_births.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_birth_keys, h->h_birth_keys.data(), (size_t)K * sizeof(long long), hipMemcpyHostToDevice, s);
    return e;
}
// The activation itself, shared by a single handle's births (births_end) and a shard's (mvhdp_activate_births): every (topic, key) of
// `born` -- checked by the caller, in index order -- leaves inActiveTopicIndex and its alpha[view(key)][k] takes alpha[view(key)][K]
// (UPD:263-270); the F+trees of the old alpha are no longer current.
int activate_born(mvhdp_ctx* h, const std::vector<std::pair<int32_t, long long>>& born, SweepOutcome& oc)
{
    if (born.empty()) return MVHDP_OK;
    MvModel& mm = h->mm;
    const int K = mm.K;
    for (const auto& b : born) {
        const int t = b.first, mv = MVHDP_ACT_KEY_VIEW(b.second);
        h->h_inactive[t] = 0;
        h->h_alpha[(size_t)mv * (K + 1) + t] = h->h_alpha[(size_t)mv * (K + 1) + K];
        if (oc.n_activations++ == 0) oc.first_act = b.second;
    }
    mm.first_inactive = -1;
    for (int k = 0; k < K; k++) if (h->h_inactive[k]) { mm.first_inactive = k; break; }
    h->st.trees_outdated();
    HIPC(h, hipMemcpy(h->d_alpha, h->h_alpha.data(), h->h_alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMemcpy(h->d_inactive, h->h_inactive.data(), (size_t)K, hipMemcpyHostToDevice));
    return MVHDP_OK;
}

static int births_end(mvhdp_ctx* h, hipStream_t s, SweepOutcome& oc)
{
    MvModel& mm = h->mm;
    const int K = mm.K;
    int32_t head[2] = {0, 0};
    HIPC(h, hipMemcpyAsync(head, h->d_births, sizeof head, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    const int n = std::min(head[0], std::min(head[1], K));
    if (n <= 0) return MVHDP_OK;
    HIPC(h, hipMemcpy(h->h_birth_keys.data(), h->d_birth_keys, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<std::pair<int32_t, long long>> born;
    for (int r = 0; r < n; r++) {
        const int t = h->h_births[(size_t)2 + r];
        const long long key = h->h_birth_keys[(size_t)r];
        if (t < 0 || t >= K || key == LLONG_MAX || !h->h_inactive[t]) continue;          // (cannot happen: position r is passed only by a delta that reached it)
        const int mv = MVHDP_ACT_KEY_VIEW(key);
        if (mv < 0 || mv >= mm.M) FAIL(h, MVHDP_ERR_STATE, "births: bad activation key");
        born.emplace_back(t, key);
    }
    return activate_born(h, born, oc);
}

// Does this sweep give birth chunk by chunk (SweepLaunch::births)?  A live sweep in its live-rows form over a truncated HDP that applies
// its own deltas; with NO_APPLY only when a document shard asks for it (MVHDP_SWEEP_SHARD_BIRTHS)
static bool sweep_births(const SweepPlan& p, uint32_t flags, const MvModel& mm)
{
    const bool shard = (flags & MVHDP_SWEEP_SHARD_BIRTHS) != 0;
    return p.live_rows && (!(flags & MVHDP_SWEEP_NO_APPLY) || shard) && mm.first_inactive >= 0 && p.only_seg < 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The sweep: plan (mvhdp_plan.h, pure) -> enqueue (launches only, nothing waits) -> finish (one synchronisation:
// statistics, the next plan's histograms, the walk search).
// ---------------------------------------------------------------------------------------------------------------
static int ensure_slot_counts(mvhdp_ctx* h)
{
    // MvModel::nslots and the histograms come from the sweep kernels themselves; after assignments arrived from the host (or an
    // entity was abandoned, Q11) they are recounted from z: one pass
    MvModel& mm = h->mm;
    if (mm.D > 0 && !h->d_nslots) {
        HIPC(h, hipMalloc(&h->d_nslots, (size_t)mm.D * sizeof(uint16_t)));
        mm.nslots = h->d_nslots;
        h->st.nslots_invalidated();
    }
    if (h->st.nslots_valid()) return MVHDP_OK;
    unsigned long long hist[MVHDP_HIST_BINS + MVHDP_ENT_BINS] = {0};
    HIPC(h, hipMemsetAsync(h->d_ovf_meta, 0, META_BYTES, h->stream));
    HIPC(h, mvhdp_launch_slot_hist(mm, (unsigned long long*)h->d_ovf_meta + META_HIST, h->stream));
    HIPC(h, hipMemcpyAsync(hist, (unsigned long long*)h->d_ovf_meta + META_HIST, sizeof hist, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::copy(hist, hist + MVHDP_HIST_BINS, h->last_hist);
    std::copy(hist + MVHDP_HIST_BINS, hist + MVHDP_HIST_BINS + MVHDP_ENT_BINS, h->last_ent);
    h->st.nslots_counted(true);
    return MVHDP_OK;
}

static void fill_plan_in(mvhdp_ctx* h, uint32_t flags, bool debug, bool batch, PlanIn& in)
{
    const MvModel& mm = h->mm;
    in.K = mm.K; in.M = mm.M; in.D = mm.D;
    in.mdt = compute_max_doc_tokens(h);
    in.have_order = h->d_doc_order != nullptr && !h->tokens_desc.empty();
    for (int c = 0; c < 5; c++)
        in.n_longer[c] = in.have_order ? (int64_t)(std::upper_bound(h->tokens_desc.begin(), h->tokens_desc.end(), (int64_t)64 << c, std::greater<int64_t>()) - h->tokens_desc.begin()) : mm.D;
    std::copy(h->last_hist, h->last_hist + MVHDP_HIST_BINS, in.tok_hist);
    std::copy(h->last_ent, h->last_ent + MVHDP_ENT_BINS, in.ent_hist);
    in.flags = flags; in.debug = debug; in.batch = batch;
    in.trees_current = h->st.trees_current();
    in.unassigned = h->st.any_unassigned();
    in.first_inactive = mm.first_inactive;
    in.vectors_mix = mm.mix != nullptr && !(flags & MVHDP_SWEEP_FROZEN);      // (the inferencer's worker has lambda = 0: INF:251-252)
    in.num_cus = h->num_cus; in.max_lds = h->max_lds;
    in.regs = h->regs;
    in.slim_table = mm.counts12 != nullptr;
    in.max_types = 0;
    for (int m = 0; m < mm.M; m++) in.max_types = std::max(in.max_types, (int)mm.V[m]);
}

static int alloc_debug(mvhdp_ctx* h, const mvhdp_debug* dbg, DebugBufs& db)
{
    const int K = h->mm.K, M = h->mm.M;
    hipStream_t s = h->stream;
    for (int m = 0; m < M; m++) {
        if (dbg->tok_dbg[m] && h->N[m] > 0) {
            void* p = nullptr;
            hipError_t e = hipMalloc(&p, (size_t)h->N[m] * 4 * sizeof(double));
            if (e != hipSuccess) { db.release(); HIPC(h, e); }
            db.to_free.push_back(p);
            hipMemsetAsync(p, 0, (size_t)h->N[m] * 4 * sizeof(double), s);
            db.tok_dbg[m] = (double*)p;
        }
    }
    if (dbg->n_trace > 0) {
        void *a = nullptr, *b = nullptr, *c = nullptr, *o = nullptr;
        const size_t n = (size_t)dbg->n_trace;
        if (hipMalloc(&a, n * 8) != hipSuccess || hipMalloc(&b, n * 4) != hipSuccess ||
            hipMalloc(&c, n * 4) != hipSuccess || hipMalloc(&o, n * (K + 1) * 8) != hipSuccess) {
            for (void* q : {a, b, c, o}) if (q) hipFree(q);
            db.release(); FAIL(h, MVHDP_ERR_HIP, "debug trace allocation failed");
        }
        db.to_free.push_back(a); db.to_free.push_back(b); db.to_free.push_back(c); db.to_free.push_back(o);
        hipMemcpyAsync(a, dbg->trace_doc, n * 8, hipMemcpyHostToDevice, s);
        hipMemcpyAsync(b, dbg->trace_view, n * 4, hipMemcpyHostToDevice, s);
        hipMemcpyAsync(c, dbg->trace_pos, n * 4, hipMemcpyHostToDevice, s);
        hipMemsetAsync(o, 0, n * (K + 1) * 8, s);
        db.n_trace = dbg->n_trace;
        db.trace_doc = (const int64_t*)a; db.trace_view = (const int32_t*)b; db.trace_pos = (const int32_t*)c;
        db.trace_out = (double*)o;
    }
    return MVHDP_OK;
}

// how many of the positions 0 .. P-1 of the longest-first order belong to segment seg (positions seg, seg + nseg, ...)
static int64_t segment_share(int64_t P, int seg, int nseg) { return P > seg ? (P - seg + nseg - 1) / nseg : 0; }

// The control words and entity lists one segment's kernels work with (a second set exists for overlapped segments: two segments in flight)
struct SegCtl {
    unsigned int* class_counts;        // [MVHDP_N_CLASSES] lengths of the route pass's lists
    unsigned long long* qheads;        // [8] one work-queue head per kernel class
    int32_t* lists;                    // [MVHDP_N_CLASSES][D] entity lists (nullptr: the handle's own, allocated on first use)
    int census_set = 0;                // the launch census' set of statistics blocks (mvhdp_ctx::Census): the second one for the second segment in flight
};

// Route pass + every class kernel of segment `seg` on stream s (the wider classes on the side streams behind a fork event, joined
// back into s): positions seg, seg + nseg, ... of the longest-first order.  mk = the model these kernels read and update.
static hipError_t launch_segment_kernels(mvhdp_ctx* h, const SweepPlan& p, const MvModel& mk_in, const SweepLaunch& sl, int seg, hipStream_t s,
                                         const SegCtl& ctl, unsigned long long* d_stats)
{
    const MvModel& mm = h->mm;
    MvModel mk = mk_in;
    if (p.frozen) { mk.mix = nullptr; mk.mix32 = nullptr; }                       // a FROZEN sweep samples without the mix (INF:251-252): the plain kernels
    const int nseg = p.nseg;
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    auto share = [&](int64_t P) { return segment_share(P, seg, nseg); };
    const int64_t n_seg = share(mm.D);
    unsigned int* class_counts = ctl.class_counts;
    // entities a class kernel of this segment is sized for (an upper bound is enough: the queue is dynamic)
    double tok_tot = 0;
    for (int b = 0; b < MVHDP_HIST_BINS; b++) tok_tot += (double)h->last_hist[b];
    const bool sizes_known = h->last_ent[MVHDP_N_CLASSES] == 0 && tok_tot > 0;
    auto blocks_for = [&](int64_t n, const ClassLaunch& g) {
        const int64_t need = (n + (int64_t)g.wpb * MVHDP_DOC_BATCH - 1) / ((int64_t)g.wpb * MVHDP_DOC_BATCH);
        return (int)std::max<int64_t>(1, std::min<int64_t>(need, g.grid));
    };
    {
        const int64_t H_seg = p.route ? share(p.H) : 0;
        ClassifyArgs ca{};
        int32_t* lists = ctl.lists ? ctl.lists : h->d_lists;
        bool used_stream[PLAN_N_STREAMS] = {};
        // the launch census: a zeroed block per class launch instead of the sweep's counters, folded into them behind the join events below.
        // This set's last fold sits in front of this on the same stream.
        CensusFold cf{};
        unsigned long long* census_blocks = nullptr;
        if (h->census.on) {
            census_blocks = h->census.d_blocks + (size_t)ctl.census_set * MVHDP_N_CLASSES * ST_COUNT;
            step(hipMemsetAsync(census_blocks, 0, (size_t)MVHDP_N_CLASSES * ST_COUNT * sizeof(unsigned long long), s));
            cf.blocks = census_blocks; cf.stats = d_stats; cf.tally = h->census.d_tally;
        }
        if (p.route && H_seg > 0) {
            if (!ctl.lists && !h->d_lists) step(hipMalloc(&h->d_lists, (size_t)MVHDP_N_CLASSES * mm.D * sizeof(int32_t)));
            lists = ctl.lists ? ctl.lists : h->d_lists;
            if (!h->ev_fork) step(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
            if (e != hipSuccess) return e;
            ca.order = h->d_doc_order; ca.n = H_seg; ca.start = seg; ca.stride = nseg;
            for (int c = 0; c < MVHDP_N_CLASSES; c++) { ca.class_map[c] = p.class_map[c]; ca.lists[c] = lists + (size_t)c * mm.D; }
            ca.check_views = compute_max_doc_tokens(h) > 65535 ? 1 : 0;
            ca.counts = class_counts;
            // (counted with this sweep's own counters: in a batch -- mvhdp_sweep_many -- every sweep resets the shared control block,
            // its statistics slot survives to the read-back at the end)
            ca.misrouted = d_stats + ST_MISCLASS;
            step(mvhdp_launch_classify(mm, ca, s));
            step(hipEventRecord(h->ev_fork, s));
        }
        // every class kernel of the segment, the widest (longest entities: the sweep's critical path) first; the plan says on which
        // stream (the widest on the handle's own, the primary on a side stream behind the fork event, see mvhdp_plan.h)
        for (int c = MVHDP_N_CLASSES - 1; c >= p.pc && e == hipSuccess; c--) {
            const ClassLaunch& g = p.cls[c];
            if (!g.used) continue;
            if (c != p.pc && !(p.route && H_seg > 0)) continue;   // nothing was routed in this segment: the primary alone
            hipStream_t st = s;
            if (g.stream != PLAN_STREAM_MAIN && p.route && H_seg > 0) {
                const int si = g.stream;
                // A and B (the classes of 8 and 16 rounds): high priority = a hardware-queue pool of their own (mvhdp_plan.h)
                if (!h->side[si]) step(make_stream(&h->side[si], si != PLAN_STREAM_C && h->side_priority && !(h->side_priority == 2 && si == PLAN_STREAM_D)));
                if (!h->ev_join[si]) step(hipEventCreateWithFlags(&h->ev_join[si], hipEventDisableTiming));
                if (e != hipSuccess) return e;
                if (!used_stream[si]) step(hipStreamWaitEvent(h->side[si], h->ev_fork, 0));
                used_stream[si] = true;
                st = h->side[si];
            }
            // the side streams' kernels first: hold this stream for a moment before the primary takes the chip (mvhdp_launch_delay)
            if (c == p.pc && st == s) {
                bool side = false;
                for (int si = 1; si < PLAN_N_STREAMS; si++) side = side || used_stream[si];
                if (side) step(mvhdp_launch_delay(h->tu.fork_delay_us, s));
            }
            SweepLaunch sc = sl;
            sc.doc_counter = ctl.qheads + c;
            sc.wave_bytes = g.wave_bytes; sc.waves_per_block = g.wpb; sc.S_cap = g.S_cap;
            sc.walk = g.walk; sc.narrow = g.narrow;
            for (int m = 0; m < MVHDP_MAXM; m++) sc.walk_theta[m] = g.theta[m];
            int64_t n_c;
            if (c == p.pc) {
                // the primary: the routed entities that fit it, then everything too short to exceed it
                if (p.route && H_seg > 0) { sc.q_list = ca.lists[c]; sc.q_list_count = class_counts + c; }
                sc.q_order = h->d_doc_order; sc.q_order_start = seg + H_seg * nseg; sc.q_order_stride = nseg; sc.q_order_count = n_seg - H_seg;
                n_c = n_seg;
            } else {
                sc.q_list = ca.lists[c]; sc.q_list_count = class_counts + c;
                sc.q_order = nullptr; sc.q_order_start = 0; sc.q_order_count = 0;
                // entities this class can receive: those the plan's histogram puts there (and into classes mapped onto it), doubled
                // for the unevenness of a segment; everything of the prefix when the sizes are not known
                n_c = H_seg;
                if (sizes_known) {
                    unsigned long long cnt = 0;
                    for (int q = 0; q < MVHDP_N_CLASSES; q++) if (p.class_map[q] == c) cnt += h->last_ent[q];
                    n_c = std::min<int64_t>(H_seg, (int64_t)(2 * cnt / (unsigned)nseg) + 64);
                }
            }
            int row = -1;
            if (census_blocks) sc.stats = census_blocks + (size_t)cf.n * ST_COUNT;
            if (g.fast) step(mvhdp_launch_sweep_fast_row(mk, sc, g.r, blocks_for(n_c, g), p.debug, st, &row));
            else step(mvhdp_launch_sweep_row(mk, sc, blocks_for(n_c, g), p.debug, st, &row));
            if (census_blocks) {
                cf.row[cf.n++] = row;
                if (row >= 0) h->census.launches[row]++;
            }
        }
        for (int si = 1; si < PLAN_N_STREAMS; si++) if (used_stream[si]) step(hipEventRecord(h->ev_join[si], h->side[si]));
        for (int si = 1; si < PLAN_N_STREAMS; si++) if (used_stream[si]) step(hipStreamWaitEvent(s, h->ev_join[si], 0));
        if (census_blocks) { const hipError_t ef = mvhdp_launch_census_fold(cf, s); step(ef); }   // (whatever failed above: what did run is counted)
    }
    return e;
}

// ---- What the two ways of putting a sweep on the device share (enqueue_sweep: one segment after the other; enqueue_overlapped: two in
// flight): the kernels' arguments, the view weights, the trees a sweep starts with, the end of a live sweep.  The handle's flags are set
// whether or not a launch failed, as every launch is attempted: the first error is what the caller reports. ----

// The arguments every class kernel of the sweep receives (launch_segment_kernels adds the class's own), from the plan alone
static SweepLaunch fill_launch(mvhdp_ctx* h, const SweepPlan& p, uint32_t sweep_idx, uint64_t seed, const DebugBufs* db, unsigned long long* d_stats)
{
    SweepLaunch sl{};
    sl.sweep_idx = sweep_idx; sl.seed_lo = (uint32_t)seed; sl.seed_hi = (uint32_t)(seed >> 32);
    sl.flags = p.flags & 0x7fffu; sl.S_cap = p.S_cap;
    if (h->tu.single_wave && p.live) sl.flags |= MVHDP_SL_STRICT_LIVE;
    if (p.live_rows && h->diag.no_row_sample) sl.flags |= MVHDP_SL_NO_ROW_SAMPLE;                // (measurement only: what the tree branch's row scan costs)
#ifdef MVHDP_PROBE
    if (!p.overlap)                                                                              // (two segments in flight never took the probe)
        if (const char* f = getenv("MVHDP_ATOMIC_PROBE")) sl.flags |= ((unsigned)atoi(f) & 7u) << 16;     // measurement build only (mvhdp_sweep_fast.hip)
#endif
    sl.q_order_stride = 1;
    sl.nk_global = p.nk_global; sl.block_shared_bytes = p.block_shared_bytes;
    sl.live16 = p.live16 ? 1 : 0; sl.delta16 = p.delta16 ? 1 : 0;
    sl.live_rows = p.live_rows ? 1 : 0; sl.coef_lds = p.coef_lds ? 1 : 0;
    sl.stats = d_stats; sl.act_key = h->d_act_key;
    if (sweep_births(p, p.flags, h->mm)) { sl.births = h->d_births; sl.birth_keys = h->d_birth_keys; }   // born chunk by chunk (births_begin / births_end), not one per segment
    sl.slot_hist = (unsigned long long*)h->d_ovf_meta + META_HIST;
    if (db) {
        for (int m = 0; m < h->mm.M; m++) sl.tok_dbg[m] = db->tok_dbg[m];
        sl.n_trace = db->n_trace; sl.trace_doc = db->trace_doc; sl.trace_view = db->trace_view; sl.trace_pos = db->trace_pos; sl.trace_out = db->trace_out;
    }
    return sl;
}

// The view weights p[d][m][m'] of this sweep: the host's, or drawn on the device.
// (drawing them on a stream of their own beside the tree rebuild was tried in round 4: 0.15 ms of overlap on paper, but the
// extra stream cost a segmented sweep 0.1-0.2 ms per segment in launch latency and a deferred one nothing gained: gpurun_out/r4t)
static hipError_t view_weights(mvhdp_ctx* h, uint32_t sweep_idx, uint64_t seed, const double* p_override, hipStream_t s)
{
    MvModel& mm = h->mm;
    if (mm.M <= 1) return hipSuccess;
    const size_t bytes = (size_t)mm.D * mm.M * mm.M * sizeof(double);
    if (!mm.p && mm.D > 0) { hipError_t e = hipMalloc(&mm.p, bytes); if (e != hipSuccess) return e; }
    if (p_override) return hipMemcpyAsync(mm.p, p_override, bytes, hipMemcpyHostToDevice, s);
    return mvhdp_launch_draw_p(mm, sweep_idx, (uint32_t)seed, (uint32_t)(seed >> 32), s);
}

// live-rows form on the mirror: the heavy words keep stored trees, and a small kernel beside the samplers keeps those current
// (heavy_refresh_kernel); not with one resident wave (mvhdp_tuning.single_wave: the sequential pin has no second kernel)
static bool uses_refresher(const mvhdp_ctx* h, const SweepPlan& p) { return p.live_rows && p.live16 && !h->tu.single_wave && !h->diag.no_heavy_refresh; }

static hipError_t ensure_heavy_list(mvhdp_ctx* h)            // the list of the heavy rows and its two control words
{
    if (h->d_heavy_list) return hipSuccess;
    const hipError_t e = hipMalloc(&h->d_heavy_list, (size_t)MVHDP_HEAVY_CAP * sizeof(int32_t));
    return e != hipSuccess ? e : hipMalloc(&h->d_heavy_ctl, 2 * sizeof(unsigned int));
}
static hipError_t ensure_refresher(mvhdp_ctx* h)             // the refresher's stream and the events around its kernel
{
    if (h->rf_stream) return hipSuccess;
    hipError_t e = make_stream(&h->rf_stream, true);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_rf_go, hipEventDisableTiming);
    return e != hipSuccess ? e : hipEventCreateWithFlags(&h->ev_rf_done, hipEventDisableTiming);
}

// no stored trees: the weight classes and the mirror, the coefficients and tree[1] of every word from the current counts
static hipError_t live_rows_prepare(mvhdp_ctx* h, const SweepPlan& p, bool from_mirror, hipStream_t s)
{
    hipError_t e = p.live16 ? ensure_heavy_list(h) : hipSuccess;
    if (e == hipSuccess && uses_refresher(h, p)) e = ensure_refresher(h);
    if (e != hipSuccess) return e;
    return mvhdp_launch_live_rows_prepare(h->mm, from_mirror, p.live16, p.live16 ? h->d_heavy_list : nullptr, p.live16 ? h->d_heavy_ctl : nullptr, MVHDP_HEAVY_CAP,
                                          p.live16 ? 512 : 256 /* cells of one register batch of a row: row_sample_live */, s);
}

static hipError_t rebuild_trees(mvhdp_ctx* h, const SweepPlan& p, hipStream_t s)
{
    const hipError_t e = mvhdp_launch_build_trees(h->mm, false, p.need_full, s);
    h->st.trees_built(p.need_full, false);
    return e;
}

// The trees (and the mirror) of the sweep-start counts: the live-rows form prepares its rows instead; REUSE_TREES keeps what the host
// built.  Then FTree.tree itself, if this sweep's kernels can reach the generic kernel and the last build left it out.
static hipError_t trees_at_sweep_start(mvhdp_ctx* h, const SweepPlan& p, hipStream_t s)
{
    hipError_t e = hipSuccess, e2 = hipSuccess;
    h->st.sweep_planned(p.need_full);
    if (p.live_rows) { e = live_rows_prepare(h, p, false, s); h->st.trees_overwritten(); }
    else if (!(p.flags & MVHDP_SWEEP_REUSE_TREES)) e = rebuild_trees(h, p, s);
    if (p.need_full && !h->st.full_trees()) { e2 = mvhdp_launch_build_trees(h->mm, h->st.trees_inference(), true, s); h->st.full_trees_written(); }
    return e != hipSuccess ? e : e2;
}

// The end of a live sweep: the 32-bit table is the model again (the mirror is now ahead of the trees); NO_APPLY: delta = after - before,
// counts = the snapshot; else UPD:202-215.  Trees rebuilt at a segment border belong to the live counts, not to the snapshot NO_APPLY restores,
// and those of overlapped segments sit in either table set.  (After a serial sweep that applies its deltas, mvhdp_sweep_finish / _many clear the flag.)
static hipError_t live_epilogue(mvhdp_ctx* h, const SweepPlan& p, unsigned long long* d_stats, hipStream_t s)
{
    MvModel& mm = h->mm;
    const bool no_apply = (p.flags & MVHDP_SWEEP_NO_APPLY) != 0;
    hipError_t e = hipSuccess;
    if (p.live16 && mm.D > 0) { e = mvhdp_launch_widen_mirror(mm, s); h->st.trees_outdated(); }
    const hipError_t e2 = mvhdp_launch_live_helper(mm, no_apply ? 1 : 2, d_stats, s);
    if (p.nseg > 1 && !(p.flags & MVHDP_SWEEP_REUSE_TREES) && (no_apply || p.overlap)) h->st.trees_outdated();
    return e != hipSuccess ? e : e2;
}

// ---------------------------------------------------------------------------------------------------------------
// Overlapped segments: two segments of a sweep in flight, so that no segment border idles the chip (a segment's kernels end with
// a tail of one entity's time per wave, and the updater's pass and the tree rebuild used to run alone between two segments).
//
//   MVHDP_SWEEP_SEGMENT_APPLY | SEGMENT_OVERLAP (deterministic, the oracle follows it)
//     The counts (and their 16-bit mirror) are kept twice (B0/B1) and the deltas in three buffers used in turn.  Segment s samples
//     against the copy that holds the deltas of every segment up to s-2 and writes its own deltas into buffer s mod 3; when its
//     kernels are done the updater's kernel A(s) -- beside the kernels of segment s+1 -- adds the deltas of segments s-1 and s to the
//     OTHER copy; segment s+2 waits for A(s).  At the end the copy that missed the last segment takes it, and both copies are the
//     model again.  The F+trees are those of the sweep start for EVERY segment while n_wk and n_k advance: this DEVIATES from the reference,
//     whose updater refreshes the two touched leaves with every delta (UPD:242-260 -> FT:138-147), so that its trees track the counts --
//     here the tree-branch mass of a token and the count-based branch come from different model states, and the LL curves price that at
//     about half a reference sweep per sweep.  Rebuilding the trees per segment beside the samplers took a whole
//     segment's time in the one block slot per CU the samplers leave (profiles/r04_timeline_c4_oseg8_trees_per_segment.txt), which put
//     the rebuild back on the critical path; the mode is opt-in for a host that knows its tree branch to be small.
//         stream 0:  K(0) A(0) K(2) A(2) K(4) ...          A(s) behind K(s) on its stream and behind A(s-1) on the other one;
//         stream 1:  K(1) A(1) K(3) A(3) ...               K(s+2) behind A(s): while A(s) runs, stream 1 - s mod 2 is sampling
//   MVHDP_SWEEP_LIVE (racy by design, like the reference's updater)
//     One copy of the counts, updated in place; only the descent tables exist twice.  The trees of segment s+1 are rebuilt from the
//     live counts when segment s is about three fifths through (a one-wave gate kernel watches its work-queue head), into the tables
//     segment s-1 has finished with, and segment s+1's kernels follow at once: its first blocks fill in as segment s drains.
// The class kernels' grids leave one block per CU free (SweepPlan::overlap): the updater / tree kernels and the next segment's first
// blocks always find room.  No kernel ever waits for another one on the device (dependencies are stream events; the gate watches a
// kernel that itself waits for nothing), so nothing here can deadlock.
// ---------------------------------------------------------------------------------------------------------------
static int ensure_overlap_buffers(mvhdp_ctx* h, const SweepPlan& p)
{
    MvModel& mm = h->mm;
    const int64_t nrows = mm.rowbase[mm.M];
    const size_t cbytes = (size_t)(counts_len(h) + MVHDP_TAIL_WORDS) * sizeof(int32_t);
    auto& ov = h->ov;
    if (!ov.x1) HIPC(h, hipStreamCreateWithFlags(&ov.x1, hipStreamNonBlocking));
    if (!ov.ev_start) HIPC(h, hipEventCreateWithFlags(&ov.ev_start, hipEventDisableTiming));
    while (ov.ev_seg.size() < (size_t)3 * p.nseg) { hipEvent_t ev; HIPC(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming)); ov.ev_seg.push_back(ev); }
    if (p.live) {                                        // (the trees exist twice for live sweeps only: the segmented sweep keeps the sweep-start trees)
        if (!ov.dtab2) HIPC(h, hipMalloc(&ov.dtab2, (size_t)nrows * mm.dt_nblk * 8 * sizeof(double)));
        if (!ov.root2) HIPC(h, hipMalloc(&ov.root2, (size_t)nrows * sizeof(double)));
        if (p.need_full && !ov.trees2) HIPC(h, hipMalloc(&ov.trees2, (size_t)nrows * 2 * mm.K * sizeof(double)));
    }
    if (!ov.ctl2) { HIPC(h, hipMalloc(&ov.ctl2, 16 * sizeof(unsigned long long))); HIPC(h, hipMemset(ov.ctl2, 0, 16 * sizeof(unsigned long long))); }
    if (p.route && !ov.lists2 && mm.D > 0) HIPC(h, hipMalloc(&ov.lists2, (size_t)MVHDP_N_CLASSES * mm.D * sizeof(int32_t)));
    if (p.seg_apply) {
        if (!ov.counts2) HIPC(h, hipMalloc(&ov.counts2, cbytes));
        if (!ov.counts16_2) HIPC(h, hipMalloc(&ov.counts16_2, (size_t)nrows * mm.K * sizeof(uint16_t)));
        if (!ov.delta2) { HIPC(h, hipMalloc(&ov.delta2, cbytes)); HIPC(h, hipMemset(ov.delta2, 0, cbytes)); }
        if (!ov.delta3) { HIPC(h, hipMalloc(&ov.delta3, cbytes)); HIPC(h, hipMemset(ov.delta3, 0, cbytes)); }
    }
    return MVHDP_OK;
}

static int enqueue_overlapped(mvhdp_ctx* h, const SweepPlan& p, uint32_t sweep_idx, uint64_t seed, const double* p_override,
                              unsigned long long* d_stats, hipEvent_t ev_k0, hipEvent_t ev_k1)
{
    MvModel& mm = h->mm;
    const int M = mm.M, nseg = p.nseg;
    const uint32_t flags = p.flags;
    // what the plan never combines with two segments in flight (mvhdp_plan.h, p.overlap): nothing below provides for it
    if (p.live_rows || p.coef_lds || p.debug || sweep_births(p, flags, mm) || p.only_seg >= 0)
        FAIL(h, MVHDP_ERR_HIP, "internal: overlapped segments planned together with live rows, debug outputs, births or a single segment");
    int rc = ensure_overlap_buffers(h, p); if (rc) return rc;
    auto& ov = h->ov;
    hipStream_t X[2] = {h->stream, h->diag.overlap_serial ? h->stream : ov.x1};   // (diagnostics: the same schedule on one stream)
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    const int64_t clen = counts_len(h), nrows = mm.rowbase[M];
    const size_t cbytes = (size_t)clen * sizeof(int32_t);

    const SweepLaunch sl = fill_launch(h, p, sweep_idx, seed, nullptr, d_stats);
    step(view_weights(h, sweep_idx, seed, p_override, X[0]));
    bool use_mirror = false;
    for (int c = 0; c < MVHDP_N_CLASSES; c++) use_mirror = use_mirror || (p.cls[c].used && p.cls[c].narrow);
    step(trees_at_sweep_start(h, p, X[0]));                        // what segments 0 and 1 sample from
    // the two copies of the model
    MvModel B[2] = {mm, mm};
    if (p.live) { B[1].dtab = ov.dtab2; B[1].root = ov.root2; if (ov.trees2) B[1].trees = ov.trees2; }
    int32_t* D3[3] = {mm.delta, ov.delta2, ov.delta3};
    if (p.seg_apply) {
        B[1].counts = ov.counts2; B[1].counts16 = ov.counts16_2;
        step(hipMemcpyAsync(ov.counts2, mm.counts, cbytes, hipMemcpyDeviceToDevice, X[0]));
        step(hipMemcpyAsync(ov.counts16_2, mm.counts16, (size_t)nrows * mm.K * sizeof(uint16_t), hipMemcpyDeviceToDevice, X[0]));
        if (!h->st.delta_clean()) step(hipMemsetAsync(mm.delta, 0, cbytes, X[0]));
        h->st.delta_written(false);
        if (h->st.deltas_dirty()) { step(hipMemsetAsync(ov.delta2, 0, cbytes, X[0])); step(hipMemsetAsync(ov.delta3, 0, cbytes, X[0])); }
        h->st.overlap_enqueued();                                  // (overlap_finished: mvhdp_sweep_finish / the batch's read-back, when the sweep is seen to have finished)
    } else if (flags & MVHDP_SWEEP_NO_APPLY) {                     // (live, document shards: the caller wants after - before)
        step(mvhdp_launch_live_helper(mm, 0, d_stats, X[0])); h->st.delta_written(false);
    }
    SegCtl ctl[2] = {{h->d_ovf_meta + META_CLASS_COUNTS, h->d_doc_counter, nullptr}, {(unsigned int*)(ov.ctl2 + 8), ov.ctl2, ov.lists2, 1}};
    step(mvhdp_launch_ctl_reset(d_stats, ST_COUNT, h->d_act_key, (unsigned long long*)h->d_ovf_meta, META_WORDS64, nullptr, nullptr, X[0]));
    step(hipEventRecord(ev_k0, X[0]));
    step(hipEventRecord(ov.ev_start, X[0]));
    step(hipStreamWaitEvent(X[1], ov.ev_start, 0));
    auto ev_done = [&](int s) { return ov.ev_seg[(size_t)3 * s]; };
    auto ev_applied = [&](int s) { return ov.ev_seg[(size_t)3 * s + 1]; };
    auto ev_reset = [&](int s) { return ov.ev_seg[(size_t)3 * s + 2]; };

    for (int seg = 0; seg < nseg && e == hipSuccess && mm.D > 0; seg++) {
        hipStream_t xs = X[seg & 1];
        const SegCtl& cs = ctl[seg & 1];
        MvModel mk;
        if (p.seg_apply) {
            // segment s reads the copy updated by A(s-2): copy 0 for segments 0 and 1, then (s-1) mod 2; its deltas go to buffer s mod 3
            // (A(seg - 2) sits in front of this segment on the same stream)
            mk = B[seg == 0 ? 0 : (seg - 1) & 1];
            mk.delta = D3[seg % 3];
        } else {
            // live: the counts are one; the trees of segment s are rebuilt, from the live counts, when segment s-1 is nearly through
            mk = mm;
            mk.delta = mm.counts;
            mk.dtab = B[seg & 1].dtab; mk.root = B[seg & 1].root; mk.trees = B[seg & 1].trees;
            if (seg >= 1 && !(flags & MVHDP_SWEEP_REUSE_TREES)) {
                step(hipStreamWaitEvent(xs, ev_reset(seg - 1), 0));          // (the head the gate watches has been reset for segment s-1)
                const int64_t n_prev = segment_share(mm.D, seg - 1, nseg), H_prev = p.route ? segment_share(p.H, seg - 1, nseg) : 0;
                // (three fifths through: the rebuild takes about a millisecond beside the samplers, and the next segment's first blocks
                // should be waiting when the current segment's queue runs dry)
                const unsigned long long thr = (unsigned long long)((n_prev - H_prev) * h->gate_pct / 100);
                step(mvhdp_launch_gate(ctl[(seg - 1) & 1].qheads + p.pc, thr, xs));
                MvModel tm = mm;
                tm.dtab = mk.dtab; tm.root = mk.root; tm.trees = mk.trees;
                if (p.live16) step(mvhdp_launch_build_trees_from_mirror(tm, p.need_full, xs, true));      // (the small-register flavour: beside the samplers)
                else step(mvhdp_launch_build_trees(tm, false, p.need_full, xs, true));
            } else if (seg >= 1) {
                mk.dtab = mm.dtab; mk.root = mm.root; mk.trees = mm.trees;     // REUSE_TREES: the host's trees, for every segment
            }
        }
        step(mvhdp_launch_ctl_reset(nullptr, 0, nullptr, nullptr, 0, cs.class_counts, cs.qheads, xs));
        step(hipEventRecord(ev_reset(seg), xs));
        step(launch_segment_kernels(h, p, mk, sl, seg, xs, cs, d_stats));
        step(hipEventRecord(ev_done(seg), xs));
        if (p.seg_apply) {
            // A(seg), beside the kernels of segment seg + 1: the other copy += deltas of seg - 1 and seg; its trees.  On this segment's
            // own stream, between K(seg) and K(seg + 2) -- which needs it anyway --, behind A(seg - 1) on the other stream.  (A stream
            // of its own shared a hardware queue with the side stream of the wider class kernels: the runtime has four.)
            if (seg >= 1) step(hipStreamWaitEvent(xs, ev_applied(seg - 1), 0));
            const MvModel& dst = B[(seg + 1) & 1];
            step(mvhdp_launch_apply2_counts(dst, D3[seg % 3], seg >= 1 ? D3[(seg - 1) % 3] : nullptr, use_mirror, d_stats + ST_NEGATIVE, xs));
            step(hipEventRecord(ev_applied(seg), xs));
        }
    }
    // everything back onto the handle's stream
    if (mm.D > 0 && e == hipSuccess) {
        step(hipStreamWaitEvent(X[0], p.seg_apply ? ev_applied(nseg - 1) : ev_done(nseg - 1), 0));
        if (nseg >= 2) step(hipStreamWaitEvent(X[0], ev_done(nseg - 2), 0));
        if (p.seg_apply) {
            // the copy A(nseg-1) did not write lacks the last segment's deltas
            step(mvhdp_launch_apply_sparse(B[(nseg + 1) & 1], D3[(nseg - 1) % 3], use_mirror, X[0]));
            h->st.trees_outdated();
            // (both copies equal now; copy 0 = mm is the model, every delta buffer is zero again)
        }
    }
    if (p.live) step(live_epilogue(h, p, d_stats, X[0]));
    step(hipEventRecord(ev_k1, X[0]));
    if (e != hipSuccess) HIPC(h, e);
    return MVHDP_OK;
}

// Everything one sweep puts on the device, in stream order; returns without waiting (except at the segment borders of a live /
// segmented sweep over a model with inactive topics, where the host performs the activation UPD:263-270).
// d_stats: [ST_COUNT] counters of THIS sweep; ev_k0/ev_k1: recorded around the sweep kernels.
static int enqueue_sweep(mvhdp_ctx* h, const SweepPlan& p, uint32_t sweep_idx, uint64_t seed, const double* p_override,
                         const DebugBufs* db, unsigned long long* d_stats, hipEvent_t ev_k0, hipEvent_t ev_k1, SweepOutcome& oc)
{
    if (p.overlap) return enqueue_overlapped(h, p, sweep_idx, seed, p_override, d_stats, ev_k0, ev_k1);
    MvModel& mm = h->mm;
    const int M = mm.M, nseg = p.nseg;
    const uint32_t flags = p.flags;
    hipStream_t s = h->stream;
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };

    const SweepLaunch sl = fill_launch(h, p, sweep_idx, seed, db, d_stats);
    const bool births = sl.births != nullptr;
    unsigned int* class_counts = h->d_ovf_meta + META_CLASS_COUNTS;
    step(view_weights(h, sweep_idx, seed, p_override, s));
    const bool refresher = uses_refresher(h, p);
    step(trees_at_sweep_start(h, p, s));
    // where the sweep's atomics land: the delta replica (deferred), or the shared counts themselves (live)
    MvModel mk = mm;
    if (p.live) {
        mk.delta = mm.counts;
        if (flags & MVHDP_SWEEP_NO_APPLY) { step(mvhdp_launch_live_helper(mm, 0, d_stats, s)); h->st.delta_written(false); }
    } else if (!p.frozen) {                                      // a frozen sweep queues nothing (WRK:587) and leaves the buffer alone
        if (!h->st.delta_clean()) {
            step(hipMemsetAsync(mm.delta, 0, (size_t)counts_len(h) * sizeof(int32_t), s));
            if (h->st.delta16_used()) step(hipMemsetD16Async(mm.delta16, (unsigned short)0x8000, (size_t)(mm.rowbase[M] * mm.K), s));   // (a sweep that failed before its apply pass)
            h->st.delta16_rebiased();
        }
        h->st.delta_written(p.delta16);                          // (the apply pass folds the 16-bit cells in and re-biases them)
    }
    // this sweep's counters, "no activation yet", the histograms for the next plan, the class list lengths, the queue heads: one launch
    step(mvhdp_launch_ctl_reset(d_stats, ST_COUNT, h->d_act_key, (unsigned long long*)h->d_ovf_meta, META_WORDS64, nullptr, h->d_doc_counter, s));
    if (births) step(births_begin(h, s));
    step(hipEventRecord(ev_k0, s));

    const int seg_lo = p.only_seg >= 0 ? p.only_seg : 0, seg_hi = p.only_seg >= 0 ? p.only_seg + 1 : nseg;
    for (int seg = seg_lo; seg < seg_hi && e == hipSuccess && mm.D > 0; seg++) {
        // segment seg = positions seg, seg + nseg, ... of the order
        if (seg > seg_lo) {
            // UPD:263-270 acts as soon as a delta lands on an inactive topic, and the samplers then draw the NEXT inactive
            // index (WRK:523-526): a sweep whose counts are kept current does the same at every segment border -- the
            // segment's first such delta (by entity, view, position) activates its topic before the next segment starts.
            // Not with MVHDP_SWEEP_NO_APPLY: there the caller reduces the key over all document shards first.
            if (births && !(flags & MVHDP_SWEEP_NO_APPLY) && e == hipSuccess) {
                const int rc = births_end(h, s, oc);                                     // every topic the segment's deltas reached
                if (rc != MVHDP_OK) return rc;
                mk.first_inactive = mm.first_inactive;
                step(births_begin(h, s));                                                // (an empty list once every topic is active)
                step(mvhdp_launch_ctl_reset(nullptr, 0, h->d_act_key, nullptr, 0, nullptr, nullptr, s));
            } else
            if ((p.live || p.seg_apply) && !(flags & MVHDP_SWEEP_NO_APPLY) && mm.first_inactive >= 0 && e == hipSuccess) {
                long long key = LLONG_MAX;
                step(hipMemcpyAsync(&key, h->d_act_key, sizeof key, hipMemcpyDeviceToHost, s));
                step(hipStreamSynchronize(s));
                if (e == hipSuccess && key != LLONG_MAX) {
                    const int rc = apply_activation(h, MVHDP_ACT_KEY_TOPIC(key), MVHDP_ACT_KEY_VIEW(key));
                    if (rc != MVHDP_OK) return rc;
                    if (oc.n_activations++ == 0) oc.first_act = key;
                    mk.first_inactive = mm.first_inactive;
                    step(mvhdp_launch_ctl_reset(nullptr, 0, h->d_act_key, nullptr, 0, nullptr, nullptr, s));
                }
            }
            if (p.seg_apply) {
                // the updater catches up before the next segment (UPD:197-218) and the trees follow: tokensPerTopic first (every
                // leaf needs all of it), then ONE pass per row: counts += delta, delta = 0, the row's tree and 16-bit mirror
                step(mvhdp_launch_apply_nk(mm, d_stats + ST_NEGATIVE, s));
                step(mvhdp_launch_build_trees_rows(mm, false, p.need_full, 0, mm.rowbase[M], true, d_stats + ST_NEGATIVE, s));
                h->st.trees_built(p.need_full, false);
            } else if (p.live_rows) {                                                    // tokensPerTopic has landed: new coefficients, exact roots
                step(live_rows_prepare(h, p, p.live16, s));
            } else if (p.live && !(flags & MVHDP_SWEEP_REUSE_TREES) && (h->live_tree_every <= 1 || seg % h->live_tree_every == 0)) {   // from the live counts
                if (p.live16) {                                                          // (the light rows' live counts are in the mirror)
                    step(mvhdp_launch_build_trees_from_mirror(mm, p.need_full, s));
                    h->st.trees_built(p.need_full, false);
                } else step(rebuild_trees(h, p, s));
            }
            step(mvhdp_launch_ctl_reset(nullptr, 0, nullptr, nullptr, 0, class_counts, h->d_doc_counter, s));
        }
        if (e != hipSuccess) break;
        if (refresher) {
            // the refresher starts behind the segment's prepare pass and runs beside the samplers; `stop` is set in stream order behind them
            step(hipEventRecord(h->ev_rf_go, s));
            step(hipStreamWaitEvent(h->rf_stream, h->ev_rf_go, 0));
            step(mvhdp_launch_heavy_refresh(mm, h->d_heavy_list, h->d_heavy_ctl, MVHDP_HEAVY_CAP, MVHDP_REFRESH_BLOCKS, h->rf_stream));
            step(hipEventRecord(h->ev_rf_done, h->rf_stream));
        }
        step(launch_segment_kernels(h, p, mk, sl, seg, s, SegCtl{class_counts, h->d_doc_counter, nullptr}, d_stats));
        if (refresher) {
            // (whatever failed above, the stop word is written and the refresher waited for: it also ends by itself after two seconds)
            hipError_t e2 = mvhdp_launch_set_u32(h->d_heavy_ctl + 1, 1u, s);
            if (e2 == hipSuccess) e2 = hipStreamWaitEvent(s, h->ev_rf_done, 0);
            step(e2);
        }
    }
    if (p.seg_apply && mm.D > 0) {                               // the last segment's deltas (the trees are rebuilt by whoever needs them next)
        step(mvhdp_launch_apply_delta(mm, d_stats, s));
        h->st.trees_outdated();
    }
    if (p.live) step(live_epilogue(h, p, d_stats, s));
    step(hipEventRecord(ev_k1, s));
    if (e != hipSuccess) HIPC(h, e);
    return MVHDP_OK;
}

static void stats_from_counters(const unsigned long long* hs, long long act, mvhdp_sweep_stats& st)
{
    st = mvhdp_sweep_stats{};
    st.tokens = (int64_t)hs[ST_TOKENS]; st.changed = (int64_t)hs[ST_CHANGED];
    st.new_mass_cnt = (int64_t)hs[ST_NEW]; st.topic_doc_mass_cnt = (int64_t)hs[ST_DOC];
    st.word_ftree_mass_cnt = (int64_t)hs[ST_TREE]; st.oov_skipped = (int64_t)hs[ST_OOV];
    st.aborted_docs = (int64_t)hs[ST_ABORT]; st.exact_fallbacks = (int64_t)hs[ST_FALLBACK];
    st.activation_key = act;
    st.activated_topic = -1; st.activated_modality = -1;
    if (act != LLONG_MAX) { st.activated_topic = MVHDP_ACT_KEY_TOPIC(act); st.activated_modality = MVHDP_ACT_KEY_VIEW(act); }
}

// after the synchronisation: what the sweep(s) left for the next plan, and the walk search
static void learn_from_sweep(mvhdp_ctx* h, const SweepPlan& p, const unsigned long long* hs, const unsigned long long* meta_hist, double kernel_ms, bool comparable)
{
    const MvModel& mm = h->mm;
    bool any_walk = false;
    for (int c = 0; c < MVHDP_N_CLASSES; c++) any_walk = any_walk || (p.cls[c].used && p.cls[c].walk);
    WalkTuner& wt = walk_tuner_of(h, p.flags);
    if (any_walk) wt.measured(mm.M, p.nseg, hs + ST_VIEW_BASE);
    if (mm.D > 0 && p.only_seg >= 0) {
        // a single segment was swept: its histograms describe a part of the entities only -- the earlier ones stay (every plan of
        // a single-segment sweep launches whatever is reachable), only an abandoned entity asks for a recount
        if (meta_hist[MVHDP_HIST_BINS + MVHDP_N_CLASSES] != 0) h->st.nslots_invalidated();
    } else if (mm.D > 0) {
        std::copy(meta_hist, meta_hist + MVHDP_HIST_BINS, h->last_hist);
        std::copy(meta_hist + MVHDP_HIST_BINS, meta_hist + MVHDP_HIST_BINS + MVHDP_ENT_BINS, h->last_ent);
        h->st.nslots_counted(h->last_ent[MVHDP_N_CLASSES] == 0);      // an abandoned entity (Q11): its list is recounted before the next sweep
    }
    if (h->dbg_env) {
        fprintf(stderr, "[mvhdp] walk threshold %.2f (base %.2f, phase %d, dir %+d, group %d); tree branch %.4f of tokens, walked on demand %.4f; per view tree share:",
                (double)wt.walk_probe_i / MVHDP_WALK_BINS, (double)wt.walk_i / MVHDP_WALK_BINS, wt.walk_phase, wt.walk_dir, wt.walk_cls,
                (double)hs[ST_TREE] / std::max<double>(1.0, (double)hs[ST_TOKENS]), (double)hs[ST_ONDEMAND] / std::max<double>(1.0, (double)hs[ST_TOKENS]));
        for (int m = 0; m < mm.M; m++) {
            const double n = std::max<double>(1.0, (double)hs[ST_VIEW_BASE + m * MVHDP_VIEW_STATS]);
            fprintf(stderr, " %.3f", hs[ST_VIEW_BASE + m * MVHDP_VIEW_STATS + 1] / n);
        }
        fprintf(stderr, "\n");
        if (hs[ST_T_TOTAL])
            fprintf(stderr, "[mvhdp] wave cycles: queue %.1f%% prologue %.1f%% view setup %.1f%% chunk head %.1f%% tokens %.1f%% chunk end %.1f%% | %.0f cycles per token per wave\n",
                    100.0 * hs[ST_T_QUEUE] / hs[ST_T_TOTAL], 100.0 * hs[ST_T_PROLOGUE] / hs[ST_T_TOTAL], 100.0 * hs[ST_T_VIEW] / hs[ST_T_TOTAL],
                    100.0 * hs[ST_T_CHUNK_HEAD] / hs[ST_T_TOTAL], 100.0 * hs[ST_T_TOKENS] / hs[ST_T_TOTAL], 100.0 * hs[ST_T_CHUNK_END] / hs[ST_T_TOTAL],
                    (double)hs[ST_T_TOTAL] / std::max<double>(1.0, (double)hs[ST_TOKENS]));
        if (hs[ST_T_ROWS])
            fprintf(stderr, "[mvhdp] live rows: %.0f cycles per tree-branch token, %.0f of them until the row is there (%.1f%% of the waves' time; %llu such tokens)\n",
                    (double)hs[ST_T_ROWS] / std::max<double>(1.0, (double)hs[ST_ONDEMAND]), (double)hs[ST_T_ROWS_WAIT] / std::max<double>(1.0, (double)hs[ST_ONDEMAND]),
                    100.0 * hs[ST_T_ROWS] / hs[ST_T_TOTAL], hs[ST_ONDEMAND]);
        if (hs[ST_N_WAVES])
            fprintf(stderr, "[mvhdp] cycles per token in a wave's first / second / later entities: %.0f / %.0f / %.0f (tokens %llu / %llu / %llu); per wave: block init %.0f cycles, wait + flush at the end %.0f, whole wave %.0f\n",
                    (double)hs[ST_T_ENT0] / std::max<double>(1.0, (double)hs[ST_N_ENT0]), (double)hs[ST_T_ENT1] / std::max<double>(1.0, (double)hs[ST_N_ENT1]),
                    (double)hs[ST_T_ENT2] / std::max<double>(1.0, (double)hs[ST_N_ENT2]), hs[ST_N_ENT0], hs[ST_N_ENT1], hs[ST_N_ENT2],
                    (double)hs[ST_T_INIT] / hs[ST_N_WAVES], (double)hs[ST_T_FLUSH] / hs[ST_N_WAVES], (double)hs[ST_T_TOTAL] / hs[ST_N_WAVES]);
    }
    const double tokens = (double)hs[ST_TOKENS];
    wt.observe(comparable && tokens > 0, p.walk_cfg, mm.M, tokens > 0 ? kernel_ms * 1e6 / tokens : 0.0);
}

static void debug_print_plan(const mvhdp_ctx* h, const SweepPlan& p, uint32_t sweep_idx)
{
    double tot = 0, b1 = 0, b2 = 0;                           // token share by topic-list size: <= 64, <= 128 slots
    for (int b = 0; b < MVHDP_HIST_BINS; b++) { tot += (double)h->last_hist[b]; if (b < 1) b1 += (double)h->last_hist[b]; if (b < 2) b2 += (double)h->last_hist[b]; }
    fprintf(stderr, "[mvhdp] sweep %u: %s primary class %d, routed prefix %lld, S_cap %d, %d segment(s); tokens in lists <=64: %.4f <=128: %.4f; kernels:",
            sweep_idx, p.fast ? "register-resident" : "generic", p.pc, (long long)p.H, p.S_cap, p.nseg, b1 / std::max(1.0, tot), b2 / std::max(1.0, tot));
    for (int c = 0; c < MVHDP_N_CLASSES; c++)
        if (p.cls[c].used)
            fprintf(stderr, " [class %d %s grid %d wpb %d lds %zu stream %d%s%s theta0 %.2f ents %llu]", c, p.cls[c].fast ? "fast" : "generic", p.cls[c].grid, p.cls[c].wpb, p.cls[c].lds,
                    p.cls[c].stream, p.cls[c].walk ? " walk" : "", p.cls[c].narrow == 2 ? " slim" : p.cls[c].narrow ? " narrow" : "", p.cls[c].theta[0], (unsigned long long)h->last_ent[c]);
    fprintf(stderr, "\n");
}

static int sweep_preconditions(mvhdp_ctx* h, uint32_t flags)
{
    // (before the state checks: a flag combination that can never run is an argument error, whatever the handle's state)
    if ((flags & MVHDP_SWEEP_SHARD_BIRTHS) && (!(flags & MVHDP_SWEEP_LIVE) || (flags & MVHDP_SWEEP_FROZEN) || (flags >> 24) != 0))
        FAIL(h, MVHDP_ERR_INVALID_ARG, "sweep: SHARD_BIRTHS goes with LIVE, not with FROZEN or ONLY_SEGMENT");
    int rc = require_corpus(h); if (rc) return rc;
    if (!h->have_hyper) FAIL(h, MVHDP_ERR_STATE, "sweep before set_hyper");
    if (!h->st.have_counts()) FAIL(h, MVHDP_ERR_STATE, "sweep before build_counts/set_counts");
    if ((flags & (MVHDP_SWEEP_REUSE_TREES | MVHDP_SWEEP_FROZEN)) && !h->st.trees_current()) FAIL(h, MVHDP_ERR_STATE, "REUSE_TREES / FROZEN without trees");
    if (h->st.bracket_open()) FAIL(h, MVHDP_ERR_STATE, "sweep: an mvhdp_apply_delta_begin bracket is open (call mvhdp_apply_delta_end)");
    if (h->st.delta_pending() && !(flags & MVHDP_SWEEP_FROZEN))
        FAIL(h, MVHDP_ERR_STATE, "sweep: the previous NO_APPLY sweep's deltas have not been applied (mvhdp_apply_delta)");
    if (h->st.counts_stale() && !(flags & MVHDP_SWEEP_FROZEN))
        FAIL(h, MVHDP_ERR_STATE, "sweep: the assignments were replaced after the counts were built (call mvhdp_build_counts, mvhdp_set_counts or mvhdp_counts_written first)");
    return MVHDP_OK;
}

static int set_generic_lds(mvhdp_ctx* h, const SweepPlan& p)
{
    size_t lds = 0;                                          // the generic kernel may need > 64 KiB of dynamic LDS
    for (int c = 0; c < MVHDP_N_CLASSES; c++) if (p.cls[c].used && !p.cls[c].fast) lds = std::max(lds, p.cls[c].lds);
    if (lds > 65536 && lds > h->lds_attr_set) { HIPC(h, mvhdp_sweep_set_max_lds(lds)); h->lds_attr_set = lds; }
    return MVHDP_OK;
}

// the checks, the slot counts and the plan of the coming sweep (or batch of sweeps)
static int plan_checked(mvhdp_ctx* h, uint32_t sweep_idx, uint32_t flags, bool debug, bool batch, SweepPlan& p)
{
    int rc = sweep_preconditions(h, flags); if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    rc = ensure_slot_counts(h); if (rc) return rc;
    PlanIn in; fill_plan_in(h, flags, debug, batch, in);
    plan_sweep(in, h->tu, walk_tuner_of(h, flags), p);
    if (p.err) FAIL(h, p.err, p.msg);
    rc = set_generic_lds(h, p); if (rc) return rc;
    if (h->dbg_env) debug_print_plan(h, p, sweep_idx);
    return MVHDP_OK;
}

int mvhdp_sweep_begin(mvhdp_ctx* h, uint32_t sweep_idx, uint64_t seed, uint32_t flags, const double* p_override, const mvhdp_debug* dbg, PendingSweep& ps)
{
    ps.flags = flags; ps.dbg = dbg; ps.debug = dbg != nullptr; ps.oc = SweepOutcome();
    int rc = plan_checked(h, sweep_idx, flags, ps.debug, false, ps.p); if (rc) return rc;
    hipStream_t s = h->stream;
    if (ps.debug) { rc = alloc_debug(h, dbg, ps.db); if (rc) return rc; }
    HIPC(h, hipEventRecord(h->ev[0], s));
    ps.births = sweep_births(ps.p, flags, h->mm);                    // (as enqueue_sweep decides it)
    rc = enqueue_sweep(h, ps.p, sweep_idx, seed, p_override, ps.debug ? &ps.db : nullptr, h->d_stats, h->ev[1], h->ev[2], ps.oc);
    if (rc) { ps.db.release(); return rc; }
    hipError_t e = hipSuccess;
    // MVHDP_BUF_BIRTH_KEYS: what this shard's deltas reached, by topic, for the MIN-reduce over the shards (mvhdp_activate_births)
    if ((flags & MVHDP_SWEEP_NO_APPLY) && !ps.p.frozen)
        e = mvhdp_launch_birth_table(ps.births ? h->d_births : nullptr, h->d_birth_keys, h->d_act_key, h->mm.K, h->d_birth_table, s);
    // counters | activation key | histograms: one copy into the handle's pinned buffer, in stream order behind the kernels
    if (e == hipSuccess) e = hipMemcpyAsync(h->h_ctl, h->d_ctl, (ST_COUNT + 1 + META_WORDS64) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { ps.db.release(); HIPC(h, e); }
    ps.open = true;
    return MVHDP_OK;
}

int mvhdp_sweep_finish(mvhdp_ctx* h, PendingSweep& ps, mvhdp_sweep_stats* stats)
{
    if (!ps.open) FAIL(h, MVHDP_ERR_STATE, "sweep_finish without sweep_begin");
    ps.open = false;
    MvModel& mm = h->mm;
    const SweepPlan& p = ps.p;
    const uint32_t flags = ps.flags;
    HIPC(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { ps.db.release(); HIPC(h, e); }
    const unsigned long long* hs = h->h_ctl;
    const long long act = (long long)h->h_ctl[ST_COUNT];
    const unsigned long long* meta = h->h_ctl + ST_COUNT + 1;
    if (hs[ST_MISCLASS] || meta[META_MISROUTED]) {
        ps.db.release();
        h->st.nslots_invalidated();
        FAIL(h, MVHDP_ERR_HIP, "internal: an entity reached a sweep kernel variant that cannot hold its topic list");
    }
    if (ps.debug) {
        const mvhdp_debug* dbg = ps.dbg;
        for (int m = 0; m < mm.M; m++)
            if (ps.db.tok_dbg[m] && e == hipSuccess) e = hipMemcpy(dbg->tok_dbg[m], ps.db.tok_dbg[m], (size_t)h->N[m] * 4 * sizeof(double), hipMemcpyDeviceToHost);
        if (ps.db.n_trace > 0 && e == hipSuccess) e = hipMemcpy(dbg->trace_out, ps.db.trace_out, (size_t)ps.db.n_trace * (mm.K + 1) * sizeof(double), hipMemcpyDeviceToHost);
        ps.db.release();
        if (e != hipSuccess) HIPC(h, e);
    }

    mvhdp_sweep_stats st;
    stats_from_counters(hs, act, st);
    // every entity was visited and none abandoned: no token of a known type is unassigned any more (WRK:557)
    if (!p.frozen && p.only_seg < 0 && st.aborted_docs == 0) h->st.every_token_assigned();
    const unsigned long long negatives = hs[ST_NEGATIVE];
    // (the pinned buffer belongs to the handle: a sweep begun on it before this one returns would overwrite it -- what the
    // planner learns from is copied out first)
    unsigned long long hist_keep[MVHDP_HIST_BINS + MVHDP_ENT_BINS];
    std::copy(meta + META_HIST, meta + META_HIST + MVHDP_HIST_BINS + MVHDP_ENT_BINS, hist_keep);
    unsigned long long hs_keep[ST_COUNT];
    std::copy(hs, hs + ST_COUNT, hs_keep);
    int n_activations = ps.oc.n_activations;
    int ret = MVHDP_OK;
    if (p.frozen) {
        // nothing was queued (WRK:587): the delta buffer is untouched
    } else if (flags & MVHDP_SWEEP_NO_APPLY) {
        h->st.delta_left_pending();
    } else if (p.live || p.seg_apply) {
        // the counts are already updated; what is left of the updater's work is the topic activation of the last segment
        if (p.seg_apply) h->st.delta_applied(); else h->st.trees_outdated();   // apply_delta_kernel zeroed what it added
        if (p.seg_apply && p.overlap) h->st.overlap_finished();
        if (ps.births) {                                             // the last segment's births (the earlier segments' were applied at their borders)
            ret = births_end(h, s, ps.oc);
            n_activations = ps.oc.n_activations;
        } else {
            ret = apply_activation(h, st.activated_topic, st.activated_modality);
            if (st.activated_topic >= 0) n_activations++;
        }
        if (ps.oc.first_act != LLONG_MAX) {                          // report the sweep's first activation
            st.activation_key = ps.oc.first_act;
            st.activated_topic = MVHDP_ACT_KEY_TOPIC(ps.oc.first_act); st.activated_modality = MVHDP_ACT_KEY_VIEW(ps.oc.first_act);
        }
        if (ret == MVHDP_OK && negatives) { h->err = "a topic count went below zero (UPD:202-215)"; ret = MVHDP_ERR_NEGATIVE_COUNT; }
    } else {
        if (st.activated_topic >= 0) n_activations = 1;
        ret = mvhdp_apply_delta(h, st.activated_topic, st.activated_modality);
    }
    HIPC(h, hipEventRecord(h->ev[3], s));
    HIPC(h, hipEventSynchronize(h->ev[3]));
    float ms_k = 0, ms_t = 0;
    hipEventElapsedTime(&ms_k, h->ev[1], h->ev[2]);
    hipEventElapsedTime(&ms_t, h->ev[0], h->ev[3]);
    st.sweep_kernel_ms = ms_k; st.total_ms = ms_t;
    st.activations = n_activations; st.reserved = 0;
    const bool comparable = p.fast && !ps.debug && !h->tu.walk_fixed && !(flags & (MVHDP_SWEEP_FROZEN | MVHDP_SWEEP_EXACT_CHAIN));
    learn_from_sweep(h, p, hs_keep, hist_keep, ms_k, comparable);
    if (stats) *stats = st;
    return ret;
}

extern "C" int mvhdp_sweep(mvhdp_handle h, uint32_t sweep_idx, uint64_t seed, uint32_t flags,
                           const double* p_override, const mvhdp_debug* dbg, mvhdp_sweep_stats* stats)
{
    CHECK_H(h);
    PendingSweep ps;
    const int rc = mvhdp_sweep_begin(h, sweep_idx, seed, flags, p_override, dbg, ps);
    if (rc) return rc;
    return mvhdp_sweep_finish(h, ps, stats);
}

// n sweeps (indices first_idx .. first_idx + n - 1) put on the device back to back: ONE plan, no host round trip between the
// sweeps (the iteration loop PTM:1146-1239 without its per-iteration barrier on the host), the statistics of every sweep
// collected on the device and read once.  Same integers as n calls of mvhdp_sweep: the plan decides which kernel variant visits
// an entity and when a word tree is walked, never what is sampled.  Falls back to n single calls where a sweep needs the host in
// between (inactive topics waiting for activation, view weights or debug output from the host, NO_APPLY).
extern "C" int mvhdp_sweep_many(mvhdp_handle h, uint32_t first_idx, int32_t n, uint64_t seed, uint32_t flags, mvhdp_sweep_stats* stats)
{
    CHECK_H(h);
    if (n < 0) FAIL(h, MVHDP_ERR_INVALID_ARG, "sweep_many: n < 0");
    if (n == 0) return MVHDP_OK;
    MvModel& mm = h->mm;
    const bool frozen = (flags & MVHDP_SWEEP_FROZEN) != 0;
    // (REUSE_TREES without FROZEN: the first sweep's update makes the trees stale, and a single call then says so -- MVHDP_ERR_STATE at
    // the second sweep; the batch must not sample on from stale trees and a stale mirror instead)
    if (n == 1 || mm.first_inactive >= 0 || ((flags & MVHDP_SWEEP_NO_APPLY) && !frozen) || ((flags & MVHDP_SWEEP_REUSE_TREES) && !frozen) || n > 4096) {
        for (int i = 0; i < n; i++) {
            const int rc = mvhdp_sweep(h, first_idx + (uint32_t)i, seed, flags, nullptr, nullptr, stats ? stats + i : nullptr);
            if (rc) return rc;
        }
        return MVHDP_OK;
    }
    SweepPlan p;
    int rc = plan_checked(h, first_idx, flags, false, true, p); if (rc) return rc;
    hipStream_t s = h->stream;
    if (h->stats_many_cap < n) {
        if (h->d_stats_many) { hipFree(h->d_stats_many); h->d_stats_many = nullptr; h->stats_many_cap = 0; }
        HIPC(h, hipMalloc(&h->d_stats_many, (size_t)n * ST_COUNT * sizeof(unsigned long long)));
        h->stats_many_cap = n;
    }
    while ((int)h->ev_many.size() < 2 * n) { hipEvent_t ev; HIPC(h, hipEventCreate(&ev)); h->ev_many.push_back(ev); }
    HIPC(h, hipEventRecord(h->ev[0], s));
    for (int i = 0; i < n; i++) {
        SweepOutcome oc;
        unsigned long long* d_st = h->d_stats_many + (size_t)i * ST_COUNT;
        rc = enqueue_sweep(h, p, first_idx + (uint32_t)i, seed, nullptr, nullptr, d_st, h->ev_many[2 * i], h->ev_many[2 * i + 1], oc);
        if (rc) return rc;
        if (!p.frozen && !p.live && !p.seg_apply) {
            // the updater's pass (UPD:197-218) in stream order; negative counts are counted into this sweep's counters
            HIPC(h, mvhdp_launch_apply_delta(mm, d_st, s, h->st.delta16_used()));
            h->st.delta16_rebiased();
            h->st.delta_applied();
        } else if (p.seg_apply) h->st.delta_applied();
        else if (p.live) h->st.trees_outdated();
    }
    HIPC(h, hipEventRecord(h->ev[3], s));
    std::vector<unsigned long long> hs((size_t)n * ST_COUNT);
    unsigned long long meta[META_WORDS64] = {0};
    HIPC(h, hipMemcpyAsync(hs.data(), h->d_stats_many, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPC(h, hipMemcpyAsync(meta, h->d_ovf_meta, sizeof meta, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    if (p.seg_apply && p.overlap) h->st.overlap_finished();
    float ms_t = 0;
    hipEventElapsedTime(&ms_t, h->ev[0], h->ev[3]);
    int ret = MVHDP_OK;
    double ms_sum = 0;
    for (int i = 0; i < n; i++) {
        const unsigned long long* hi = hs.data() + (size_t)i * ST_COUNT;
        mvhdp_sweep_stats st;
        stats_from_counters(hi, LLONG_MAX, st);
        float ms_k = 0;
        hipEventElapsedTime(&ms_k, h->ev_many[2 * i], h->ev_many[2 * i + 1]);
        st.sweep_kernel_ms = ms_k; st.total_ms = ms_t / n;
        ms_sum += ms_k;
        if (stats) stats[i] = st;
        if (hi[ST_MISCLASS]) { h->st.nslots_invalidated(); FAIL(h, MVHDP_ERR_HIP, "internal: an entity reached a sweep kernel variant that cannot hold its topic list"); }
        if (hi[ST_NEGATIVE] && ret == MVHDP_OK) { h->err = "a topic count went below zero (UPD:202-215)"; ret = MVHDP_ERR_NEGATIVE_COUNT; }
    }
    if (meta[META_MISROUTED]) { h->st.nslots_invalidated(); FAIL(h, MVHDP_ERR_HIP, "internal: an entity could not be routed to a sweep kernel"); }
    // the batch counts as one observation of the walk search (mean kernel time per token)
    std::vector<unsigned long long> acc(ST_COUNT, 0);
    for (int i = 0; i < n; i++) for (int k = 0; k < ST_COUNT; k++) acc[k] += hs[(size_t)i * ST_COUNT + k];
    const bool comparable = p.fast && !h->tu.walk_fixed && !(flags & (MVHDP_SWEEP_FROZEN | MVHDP_SWEEP_EXACT_CHAIN));
    learn_from_sweep(h, p, acc.data(), meta + META_HIST, ms_sum, comparable);
    if (!p.frozen && acc[ST_ABORT] == 0) h->st.every_token_assigned();
    return ret;
}

// The launch census (include/mvhdp.h).  Switching it on allocates the blocks and the tally; they stay until the handle goes.
extern "C" int mvhdp_sweep_census(mvhdp_handle h, int32_t enable, int32_t reset, mvhdp_census_row* rows, int32_t cap, int32_t* n_rows)
{
    CHECK_H(h);
    static_assert(MVHDP_CENSUS_ROWS == 60, "include/mvhdp.h says 60 rows");
    if (enable < -1 || enable > 1 || cap < 0 || (rows == nullptr && cap > 0)) FAIL(h, MVHDP_ERR_INVALID_ARG, "sweep_census: enable is -1, 0 or 1; rows with a capacity");
    auto& cs = h->census;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (enable == 1 && !cs.d_blocks) HIPC(h, hipMalloc(&cs.d_blocks, (size_t)2 * MVHDP_N_CLASSES * ST_COUNT * sizeof(unsigned long long)));
    if (enable == 1 && !cs.d_tally) {
        HIPC(h, hipMalloc(&cs.d_tally, MVHDP_CENSUS_ROWS * sizeof(unsigned long long)));
        HIPC(h, hipMemset(cs.d_tally, 0, MVHDP_CENSUS_ROWS * sizeof(unsigned long long)));
    }
    if (enable >= 0) cs.on = enable == 1;
    if (reset) {
        std::fill(cs.launches, cs.launches + MVHDP_CENSUS_ROWS, 0LL);
        if (cs.d_tally) HIPC(h, hipMemset(cs.d_tally, 0, MVHDP_CENSUS_ROWS * sizeof(unsigned long long)));
    }
    if (n_rows) *n_rows = MVHDP_CENSUS_ROWS;
    if (!rows) return MVHDP_OK;
    unsigned long long tally[MVHDP_CENSUS_ROWS] = {0};
    if (cs.d_tally) HIPC(h, hipMemcpy(tally, cs.d_tally, sizeof tally, hipMemcpyDeviceToHost));
    for (int i = 0; i < std::min<int>(cap, MVHDP_CENSUS_ROWS); i++) {
        mvhdp_census_row& r = rows[i];
        r = mvhdp_census_row{};
        if (i < MVHDP_N_FAST_FLAVOURS) {
            const FastFlavour& f = mvhdp_fast_flavours[i];
            r.rmax = f.rmax; r.debug = f.debug; r.walk = f.walk; r.narrow = f.narrow; r.roomy = f.roomy; r.liverows = f.liverows; r.mix = f.mix;
        } else {
            const int g = i - MVHDP_N_FAST_FLAVOURS;             // (mvhdp_census_generic_row: debug + 2 * mix)
            r.debug = g & 1; r.mix = g >> 1;
        }
        r.launches = cs.launches[i]; r.tokens = (int64_t)tally[i];
    }
    return MVHDP_OK;
}
