// mvhdp_census.h — the launch census (mvhdp_sweep_census): which compiled sweep kernel a class launch got, and how many tokens it
// sampled.  Host side only: no sweep kernel includes this.  One row per compiled kernel, in the order of MVHDP_FAST_FLAVOURS
// (mvhdp_flavour.h: the list the launch table of mvhdp_sweep_fast.hip is generated from as well), then the four builds of the generic
// kernel as debug + 2 * mix.
#pragma once
#include "mvhdp_device.h"

enum { MVHDP_N_GENERIC_BUILDS = 4, MVHDP_CENSUS_ROWS = MVHDP_N_FAST_FLAVOURS + MVHDP_N_GENERIC_BUILDS };
static inline int mvhdp_census_generic_row(bool debug, bool mix) { return MVHDP_N_FAST_FLAVOURS + (debug ? 1 : 0) + (mix ? 2 : 0); }

// mvhdp_launch_sweep_fast / mvhdp_launch_sweep, and *row = the census row of the kernel whose pointer the launch looked up (-1: none)
hipError_t mvhdp_launch_sweep_fast_row(const MvModel& mm, const SweepLaunch& sl, int rmax, int grid_blocks, bool debug, hipStream_t s, int* row);
hipError_t mvhdp_launch_sweep_row(const MvModel& mm, const SweepLaunch& sl, int grid_blocks, bool debug, hipStream_t s, int* row);

// The statistics blocks of one segment's class launches ([n][ST_COUNT], each launch its own) folded into the sweep's counters, and each
// block's ST_TOKENS into the tally of the row its launch took
struct CensusFold {
    const unsigned long long* blocks;
    int32_t n;
    int32_t row[MVHDP_N_CLASSES];
    unsigned long long* stats;                  // [ST_COUNT] the sweep's counters
    unsigned long long* tally;                  // [MVHDP_CENSUS_ROWS]
};
hipError_t mvhdp_launch_census_fold(const CensusFold& cf, hipStream_t s);
