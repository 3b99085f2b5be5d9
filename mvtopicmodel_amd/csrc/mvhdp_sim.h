// mvhdp_sim.h — the host-side arithmetic of mvhdp_similar_pairs as PURE functions: no HIP call, no clock, no environment.
// Reachable without a GPU through mvhdp_sim_probe (include/mvhdp.h); mvhdp_sim.hip launches exactly what these describe.
#pragma once
#include <stdint.h>
#include <cmath>

enum { SCREEN_TILE = 128,                    // the cosine screen's block tile (mvhdp_screen.h): 128 x 128 cells, 4 waves of 2 x 2 MFMA tiles of 32 x 32
       SCREEN_BK = 32,                       // its k-slab staged in LDS per step
       SIM_JSD_TILE = 16,                    // the JSD kernel's block tile (one thread per pair)
       SIM_JSD_BK = 32,                      // and its slab of topics
       SIM_MAX_DIM = 65536,                  // margin(65536) = 0.0078 < 0.01
       SIM_AUTO_STRIPE = 4096 };
static const int64_t SIM_AUTO_CAPACITY = (int64_t)1 << 22;

// margin(dim) = (dim + 4) * 2^-23.  Derived, not measured: the normalised rows a, b have sum_k |a_k b_k| <= |a||b| = 1 (up to fp64
// rounding); storing them as fp32 moves each product by at most (2 * 2^-24 + 2^-48) of itself; the fp32 fma chain of dim terms adds at
// most dim * 2^-24 * (largest partial sum <= 1 + ...) -- together below (dim + 2 + small) * 2^-24.  Taken twice over.
static inline double sim_margin(int dim) { return ((double)dim + 4.0) * std::ldexp(1.0, -23); }

static inline int sim_stripe_rows(int32_t stripe_rows) { return stripe_rows > 0 ? stripe_rows : SIM_AUTO_STRIPE; }
static inline int sim_stripes(int32_t n, int32_t stripe_rows)
{
    const int64_t S = sim_stripe_rows(stripe_rows);
    return n < 2 ? 0 : (int)((n + S - 1) / S);
}
// tile geometry of the stripe that starts at row r0: A tiles cover its rows, B tiles the columns from r0 to n, both counted from r0;
// only tiles with b >= a are computed
static inline void sim_stripe_tiles(int32_t n, int64_t r0, int64_t r1, int tile, int64_t* na, int64_t* nb)
{
    *na = (r1 - r0 + tile - 1) / tile;
    *nb = (n - r0 + tile - 1) / tile;
}
static inline int64_t sim_cells(int32_t n, int32_t stripe_rows, int tile)
{
    const int64_t S = sim_stripe_rows(stripe_rows);
    int64_t cells = 0;
    if (n < 2) return 0;
    for (int64_t r0 = 0; r0 < n; r0 += S) {
        const int64_t r1 = r0 + S < n ? r0 + S : n;
        int64_t na, nb;
        sim_stripe_tiles(n, r0, r1, tile, &na, &nb);
        for (int64_t a = 0; a < na; a++) cells += (nb - a) * (int64_t)tile * tile;
    }
    return cells;
}
