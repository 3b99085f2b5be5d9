// mvhdp_flavour.h — which compiled sweep_fast_kernel<RMAX, DEBUG, WALK, NARROW, ROOMY, LIVEROWS, MIX> a class launch gets: the rule
// (mvhdp_fast_resolve) and the list of the instantiations that exist (MVHDP_FAST_FLAVOURS), one definition each for the launch and the
// register query (mvhdp_sweep_fast.hip), the plan (mvhdp_plan.h) and the CPU test, which compiles this file with the host compiler:
// no HIP type in here.  What the flavours are, and why each is one of its own: the comment above the kernel.
#pragma once

// the flavour whose register count sizes a class's grid: PlanRegs::regs[class][.], mvhdp_sweep_kernel_regs
enum { MVHDP_FLAVOUR_PLAIN = 0, MVHDP_FLAVOUR_WALK = 1, MVHDP_FLAVOUR_DEBUG = 2, MVHDP_N_FLAVOURS = 3 };

// The widest variant with a 12-bit flavour (NARROW = 2): the 8- and 16-round variants sit at their register limit and stay on the mirror
enum { MVHDP_SLIM_MAX_ROUNDS = 4 };

// the seven template arguments, in the kernel's order
struct FastFlavour { int rmax; bool debug, walk; int narrow; bool roomy; int liverows; bool mix; };

static inline bool operator==(const FastFlavour& a, const FastFlavour& b)
{
    return a.rmax == b.rmax && a.debug == b.debug && a.walk == b.walk && a.narrow == b.narrow && a.roomy == b.roomy && a.liverows == b.liverows && a.mix == b.mix;
}

// Every instantiation, as X(RMAX, DEBUG, WALK, NARROW, ROOMY, LIVEROWS, MIX): ten for every variant, the 12-bit flavour where
// MVHDP_SLIM_MAX_ROUNDS allows it, and the 2-round variant's builds for six waves a SIMD.
#define MVHDP_FAST_FLAVOURS_OF(X, R)                                                                                   \
    X(R, false, false, 0, false, 0, false) /* plain */                                                                 \
    X(R, false, true, 0, false, 0, false)  /* thresholded walk, per-view statistics */                                 \
    X(R, true, true, 0, false, 0, false)   /* debug */                                                                 \
    X(R, false, true, 1, false, 0, false)  /* 16-bit mirror */                                                         \
    X(R, false, true, 0, false, 1, false)  /* live rows, 32-bit table */                                               \
    X(R, false, true, 1, false, 1, false)  /* live rows, mirror */                                                     \
    X(R, false, true, 1, false, 2, false)  /* live rows, mirror, rows of two batches */                                \
    X(R, false, true, 0, false, 0, true)   /* mix */                                                                   \
    X(R, true, true, 0, false, 0, true)    /* mix, debug */                                                            \
    X(R, false, true, 1, false, 0, true)   /* mix, mirror */
#define MVHDP_FAST_FLAVOURS(X)                                                                                         \
    MVHDP_FAST_FLAVOURS_OF(X, 1) MVHDP_FAST_FLAVOURS_OF(X, 2) MVHDP_FAST_FLAVOURS_OF(X, 4) MVHDP_FAST_FLAVOURS_OF(X, 8) MVHDP_FAST_FLAVOURS_OF(X, 16) \
    X(1, false, true, 2, false, 0, false) X(2, false, true, 2, false, 0, false) X(4, false, true, 2, false, 0, false)  \
    X(2, false, true, 1, true, 0, false) X(2, false, true, 2, true, 0, false) X(2, false, true, 1, true, 2, false)

#define MVHDP_FAST_FLAVOUR_KEY(R, D, W, N, RO, L, MX) {R, D, W, N, RO, L, MX},
static const FastFlavour mvhdp_fast_flavours[] = { MVHDP_FAST_FLAVOURS(MVHDP_FAST_FLAVOUR_KEY) };
enum { MVHDP_N_FAST_FLAVOURS = sizeof(mvhdp_fast_flavours) / sizeof(mvhdp_fast_flavours[0]) };

// What a class launch asks for: the class's slot rounds, the model's K, and what SweepLaunch / MvModel say
struct FastRequest {
    int rounds, K;
    bool debug, walk;                           // SweepLaunch::walk
    int narrow;                                 // SweepLaunch::narrow
    bool live_rows, live16;                     // SweepLaunch::live_rows, live16
    bool mix, counts12;                         // MvModel::mix, MvModel::counts12 set
};

// The flavour of a request, or false: a request no plan makes.  A debug launch always takes the walk flavour (a threshold of 0 walks
// every token), and the tables and the live-rows form count only with the walk flavour and without debug.
static inline bool mvhdp_fast_resolve(const FastRequest& q, FastFlavour* out)
{
    const int rmax = q.rounds == 3 ? 4 : q.rounds;
    if (rmax != 1 && rmax != 2 && rmax != 4 && rmax != 8 && rmax != 16) return false;
    const bool tables = q.walk && !q.debug;
    const int narrow = (tables && q.narrow) ? (q.narrow == 2 ? 2 : 1) : 0;
    const bool rows = tables && q.live_rows;
    // the 12-bit image: deferred sweeps without a mix, in the variants that have the flavour, on a handle that keeps the image
    if (narrow == 2 && (rmax > MVHDP_SLIM_MAX_ROUNDS || rows || q.live16 || q.mix || !q.counts12)) return false;
    // a sweep with a mix: stored trees and the walk flavour
    if (q.mix && (rows || !q.walk)) return false;
    // the 2-round variant at six waves a SIMD where a row of the mirror is 1 KiB or more; the mix flavours have no such build, and the
    // live-rows one is always that of two-batch rows (the shortcut checks the batch count at run time as well)
    const bool roomy = rmax == 2 && q.K >= 512 && narrow && !q.mix;
    const bool two_batches = narrow && (roomy || (q.K > 512 && q.K <= 1024));
    *out = FastFlavour{rmax, q.debug, q.debug || q.walk, narrow, roomy, rows ? (two_batches ? 2 : 1) : 0, q.mix};
    return true;
}
