// mvhdp_nearest.h — the host-side arithmetic of mvhdp_nearest_entities and mvhdp_topic_top_entities as PURE functions: no HIP call, no
// clock, no environment.  Reachable without a GPU through mvhdp_nearest_probe (include/mvhdp.h); mvhdp_nearest.hip launches exactly what
// these describe.
//
// Why the screen never decides.  Let b bound |screen - exact| for a pair of screened rows; sim_margin(K) (mvhdp_sim.h) is 2 b, derived
// there.  For a query row let tau be the n-th largest screen value over its screened eligible candidates.  n cells have screen >= tau, so
// their exact values are >= tau - b: the n-th largest exact value over ALL eligible candidates is >= tau - b.  Every member of the true
// first n -- ties at the n-th place included -- has an exact value >= that, hence a screen value >= tau - 2 b = tau - sim_margin(K).  So
// the cells with screen >= tau - sim_margin(K), recomputed exactly, hold the whole answer.  Any tau' <= tau gives a superset: the stripes
// of candidates are screened one after the other and a stripe is cut with the n-th largest screen value seen SO FAR (this stripe
// included), which is the tau above when one stripe holds every candidate.  Fewer than n screened cells so far: every cell passes.
#pragma once
#include <stdint.h>
#include "mvhdp_sim.h"

enum { NEAR_MAX_STRIPE = 8192,              // candidates per stripe: a stripe's 32-bit keys of one query sit in LDS (32 KiB) while tau is found
       NEAR_AUTO_BLOCK = 8192,               // queries per block
       NEAR_MAX_TOPN = 1024,                 // mvhdp_topic_top_entities: n at most
       NEAR_AUTO_SLICE = 2048 };             // mvhdp_topic_top_entities: entities one thread walks per topic
static const int64_t NEAR_SCORE_CELLS = (int64_t)1 << 26;      // the block of screen keys [block][stripe] holds at most this many (256 MiB)
static const int64_t NEAR_AUTO_CAPACITY = (int64_t)1 << 22;    // candidates of one block of queries
static const int64_t NEAR_CHUNK_BYTES = (int64_t)256 << 20;    // proportions are produced in chunks of entities of at most this size

static inline int64_t near_stripe(int32_t stripe_candidates)
{
    return stripe_candidates > 0 && stripe_candidates < NEAR_MAX_STRIPE ? stripe_candidates : NEAR_MAX_STRIPE;
}
static inline int64_t near_block(int32_t block_queries, int32_t stripe_candidates)
{
    const int64_t most = NEAR_SCORE_CELLS / near_stripe(stripe_candidates), want = block_queries > 0 ? block_queries : NEAR_AUTO_BLOCK;
    return want < most ? want : most;
}
static inline int64_t near_blocks(int64_t nq, int64_t nc, int32_t block_queries, int32_t stripe_candidates)
{
    const int64_t B = near_block(block_queries, stripe_candidates);
    return nq < 1 || nc < 1 ? 0 : (nq + B - 1) / B;
}
static inline int64_t near_tiles(int64_t rows) { return (rows + SCREEN_TILE - 1) / SCREEN_TILE; }
// matrix cells the screen computes: 128 x 128 per launched tile, every block of queries against every stripe of candidates
static inline int64_t near_cells(int64_t nq, int64_t nc, int32_t block_queries, int32_t stripe_candidates)
{
    const int64_t B = near_block(block_queries, stripe_candidates), S = near_stripe(stripe_candidates);
    int64_t cells = 0;
    if (nq < 1 || nc < 1) return 0;
    for (int64_t q0 = 0; q0 < nq; q0 += B) {
        const int64_t tq = near_tiles((q0 + B < nq ? q0 + B : nq) - q0);
        for (int64_t s0 = 0; s0 < nc; s0 += S) cells += tq * near_tiles((s0 + S < nc ? s0 + S : nc) - s0) * SCREEN_TILE * SCREEN_TILE;
    }
    return cells;
}
// mvhdp_topic_top_entities: entities per chunk of proportions and per slice of a chunk (0: auto)
static inline int64_t near_chunk(int32_t K, int64_t chunk_entities)
{
    const int64_t most = NEAR_CHUNK_BYTES / ((int64_t)K * 8) > 0 ? NEAR_CHUNK_BYTES / ((int64_t)K * 8) : 1;
    return chunk_entities > 0 && chunk_entities < most ? chunk_entities : most;
}
static inline int64_t near_slice(int64_t slice_entities) { return slice_entities > 0 ? slice_entities : NEAR_AUTO_SLICE; }
static inline int64_t near_slices(int64_t nd, int32_t K, int64_t chunk_entities, int64_t slice_entities)
{
    const int64_t C = near_chunk(K, chunk_entities), L = near_slice(slice_entities);
    int64_t n = 0;
    for (int64_t c0 = 0; c0 < nd; c0 += C) n += ((c0 + C < nd ? c0 + C : nd) - c0 + L - 1) / L;
    return n;
}
