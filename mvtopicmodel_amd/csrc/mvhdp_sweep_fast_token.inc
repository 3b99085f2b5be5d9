// One token of the register-resident sweep (WRK:425-586), included by mvhdp_sweep_fast.hip once per n_wk
// gather buffer: TOK_T = the token's position in the chunk, TOK_G = the buffer holding its gathered counts
// (refilled here for the token NB visited positions ahead).  An abandoned entity empties the mask of tokens to visit;
// tokens of types outside the vocabulary are not visited at all.
{
                    int g[RMAX];
#pragma unroll
                    for (int r = 0; r < RMAX; r++) g[r] = TOK_G[r];
                    mixg_t mg[RMAX];                                         // (MIX, view 0: mix[w][k] of the slots, gathered with the counts; else unused)
#pragma unroll
                    for (int r = 0; r < RMAX; r++) mg[r] = (MIX && mixv) ? TOK_MG[r] : (mixg_t)0;
                    // live-rows form: a token that may reach the tree branch (its u1 reaches the view's threshold) loads its word's row NOW, ahead of
                    // the next token's gather: vmcnt counts in order, and a load issued once the branch is known would wait behind that gather
                    const int wfull_t = LIVEROWS ? bcast_i(w_l, TOK_T) : 0;
                    const gptr_t rowp_t = !LIVEROWS ? (gptr_t)0 : NARROW ? scalar_row(nwk16_v, (unsigned int)W_ROW(wfull_t), (unsigned int)K * 2u)
                                                                         : scalar_row(nwk_v, (unsigned int)W_ROW(wfull_t), (unsigned int)K * 4u);
                    const bool spec_t = LIVEROWS && ((specm >> TOK_T) & 1ull);
                    const int bsel_t = (LIVEROWS == 2) ? (int)((bselm >> TOK_T) & 1ull) : 0;           // (rows of two batches: the one this token's tree branch starts in)
                    if (LIVEROWS) {
                        // (this token's gathered counts first: they were asked for a token ago and are here; waiting for them AFTER the row load
                        // is issued would mean waiting for the row load as well -- the counter is in order)
#pragma unroll
                        for (int r = 0; r < RMAX; r++) asm volatile("" : "+v"(g[r]));
                        if (spec_t) rowq = row_batch_load<(NARROW != 0)>(rowp_t, K, bsel_t, lane);
                    }
                    // the buffer is free again: gather for the token NB positions ahead.  With two buffers the
                    // gather is issued on every path and for every slot round (past the chunk's end it re-reads the
                    // last token's row; an unused round reads column 0): a fixed number of loads per token is what
                    // lets the wait at the next use be "all but the newest RMAX loads" instead of "all loads".
                    // (`rem` = the tokens still to visit, this one already taken out: the token NB ahead is its NB-th set bit)
                    const unsigned long long rem_n = (NB == 2) ? (rem & (rem - 1)) : rem;
#pragma unroll
                    for (int r = 0; r < RMAX; r++) { touch_lane_off(koff[r]); if (NARROW == 1) touch_lane_off(koffh[r]); if (NARROW == 2) touch_lane_off(kslim[r]); }
                    if (NB == 2 || LIVEROWS || rem_n) {                     // (live-rows form: always -- the wait for the token's row counts the loads issued behind it)
                        const int wn = bcast_i(w_l, rem_n ? (int)__builtin_ctzll(rem_n) : TOK_T);
                        if (NARROW == 2 && (wn & W_SLIM)) {                  // a slim row: the 12-bit image holds its counts, in fewer lines
                            const gptr_t cns = scalar_row(nwk12_v, (unsigned int)W_ROW(wn), row12_bytes);
#pragma unroll
                            for (int r = 0; r < RMAX; r++) TOK_G[r] = gather_slim(cns, kslim[r]);
                        } else if (NARROW && !(wn & W_HEAVY)) {              // a light row: the 16-bit mirror holds its counts
                            const gptr_t cnq = scalar_row(nwk16_v, (unsigned int)W_ROW(wn), (unsigned int)K * 2u);
#pragma unroll
                            for (int r = 0; r < RMAX; r++) TOK_G[r] = gather_cell<uint16_t>(cnq + (NARROW == 2 ? (unsigned int)koff[r] >> 1 : (unsigned int)koffh[r]));
                        } else {
                            const gptr_t cnp = scalar_row(nwk_v, (unsigned int)W_ROW(wn), (unsigned int)K * 4u);
#pragma unroll
                            for (int r = 0; r < RMAX; r++) TOK_G[r] = gather_cell<int32_t>(cnp + (unsigned int)koff[r]);
                        }
                        if (MIX && mixv) {                                   // view 0 with a mix: RMAX more loads, on every path through here like the counts'
                            const gptr_t mnp = scalar_row(mix_v, (unsigned int)W_ROW(wn), (unsigned int)K * (unsigned int)sizeof(mixg_t));
#pragma unroll
                            for (int r = 0; r < RMAX; r++) TOK_MG[r] = gather_mix<mixg_t>(mnp + ((unsigned int)koff[r] << MIXSH));
                        }
                    }
                    const int wcur = bcast_i(w_l, TOK_T);
                    const int w = W_ROW(wcur);                               // (a known type: the loop's mask holds no other)
                    if (NARROW == 2 && (wcur & W_SLIM)) {                    // this token's cells came from the 12-bit image: 16 bits each, the cell inside them
#pragma unroll
                        for (int r = 0; r < RMAX; r++) g[r] = slim_cell(g[r], kslim[r]);
                    }
                    const int so = bcast_i(so_l, TOK_T);
                    const int64_t row = row0 + w;

                    // WRK:434-468 decrement the local count; drop the topic when it is gone from all views
                    if (so >= 0) {                                           // slot and lane are wave-uniform: the count is read out of the
                        const int rs = so & (R_eff - 1), ls = so >> lg;      // owning lane, changed in scalar registers and written back
#pragma unroll
                        for (int r = 0; r < RMAX; r++) {
                            if (rs == r) {
                                const int c = bcast_i(cn[r], ls) - 1;
                                cn[r] = wave_writelane(cn[r], c, ls);
                                if (c == 0 && !((bcast_i((int)onz, ls) >> r) & 1)) live_m[r] &= ~(1ull << ls);
                            }
                        }
                    }

                    double mass = 0.0, s0 = 0.0, s1 = 0.0, total = 0.0;
                    int branch = 2, slot_new = -1;     // branch: 0 new-topic, 1 doc, 2 tree
                    bool unsafe = false;
                    // ---- fp32 screening (round 3) ----
                    // The kernel is bound by instruction issue (vector and scalar units both above 70 % busy), not by arithmetic width: on
                    // gfx950 an fp64 add or fma issues at the rate of an fp32 one.  What fp32 buys is FEWER instructions: a DPP scan step is
                    // one v_add_f32_dpp instead of two DPP moves and an add, the division by den is a multiplication by a reciprocal formed
                    // once per view, and two fused multiply-adds pack into one v_pk_fma_f32.  So the masses are first formed in fp32 and the
                    // reference's comparisons -- s < newMass (WRK:522), s < mass (WRK:529), cum_i >= s (WRK:531) -- decided there, with a
                    // closeness check.  Error budget, in units of 2^-24 * total: a term carries at most M + 12 roundings (beta/den: 5 -- den,
                    // a 1-ulp reciprocal, beta, their product --, the fused g/den + beta/den: 1 more; oth: M + 4 -- a pair weight, gamma*alpha, the
                    // sum with the count, M - 1 multiply-adds, the scale and its product --, pmm*cn + oth: 1 more; the product: 1), a
                    // cumulative sum at most 6 + RMAX additions on top (in-lane running sum, six scan steps, the exclusive-prefix add), and s
                    // the roundings of u1, tree[1], newMass and of the three operations that form it: below 56 for M <= 8, RMAX <= 16, so a
                    // comparison whose operands differ by more than tol = 128 * 2^-24 * total has the outcome it has in exact arithmetic,
                    // which the reference's fp64 sequence matches to 2^-45.  When any comparison is closer than that (2 to 5 tokens in 10 000 on
                    // C4 and C5: profiles/r03_screened_count.txt) the fp64 path below decides, itself certified against the sequential sum:
                    // the decisions -- hence every integer -- are the reference's, by construction.
                    // MIX, view 0: p_wt = mix + (1 - lambda) * (g + beta) / den.  (1 - lambda), rounded to fp32, is folded into the two per-slot constants
                    // -- each gains that rounding and the product's, 2 more on the longest chain: 7 for beta/den, 8 with the fused step --, then
                    // the slot's mix value rounded to fp32 (1) and its addition (1): a term carries at most M + 16 roundings, a comparison below
                    // 60 in all for M <= 8, RMAX <= 16 -- still under the 128 of tol, which stays as it is.  Every term stays non-negative
                    // (0 <= lambda <= 1, mix >= 0 and finite: mvhdp_set_vectors_mix refuses anything else), which the certified scan below rests on.
                    // The screening reads an fp32 copy of the table (MvModel::mix32, 80 MB more at C4: half the lines of a mix row per view-0 token).
                    double term[RMAX] = {};             // (fp64 terms: formed by the fp64 path only; read again by the debug trace)
                    bool need64 = DEBUG || exact_only || !SCREEN;
                    if (SCREEN && !need64) {
                        const float u1f = bcast_f(u1f_l, TOK_T), rootf = bcast_f(root32_l, TOK_T);
                        float t32[RMAX], c32v[RMAX];
#pragma unroll
                        for (int r = 0; r < RMAX; r++) {
                            float pw = __builtin_fmaf((float)g[r], rden32[r], brden32[r]);          // WRK:507: (g + beta) / den  (MIX, view 0: times 1 - lambda)
                            if (MIX && mixv) pw += (float)mg[r];                                    // WRK:504 (the cell of the fp32 copy)
                            const float a32 = __builtin_fmaf(pmm32, (float)cn[r], oth32[r]);        // WRK:509
                            t32[r] = __builtin_amdgcn_inverse_ballot_w64(live_m[r]) ? a32 * pw : 0.0f;
                        }
                        float ls = t32[0];
                        c32v[0] = ls;
#pragma unroll
                        for (int r = 1; r < RMAX; r++) { ls += t32[r]; c32v[r] = ls; }
                        const float incl = wave_incl_scan_f_dpp(ls);
                        const float excl = incl - ls;
#pragma unroll
                        for (int r = 0; r < RMAX; r++) c32v[r] = (r == RMAX - 1) ? incl : excl + c32v[r];
                        const float massf = bcast_f(incl, 63);
                        const float totalf = (newMass32 + massf) + rootf;
                        const float s0f = u1f * totalf;
                        const float tolf = totalf * 0x1.0p-17f;
                        bool close;
                        if (s0f < newMass32) {
                            branch = 0;
                            close = fabsf(s0f - newMass32) <= tolf;
                        } else {
                            const float s1f = s0f - newMass32;
                            // (s near newMass; without a new-topic mass that is s near 0, where nothing is decided -- it goes to fp64 all the
                            // same, one token in 10^5, rather than pay for a test of newMass on every token)
                            close = (fabsf(s1f) <= tolf) || (fabsf(s1f - massf) <= tolf);
                            if (s1f < massf) {
                                branch = 1;
                                unsigned long long anyhit = 0, near = 0, hitr[RMAX];
#pragma unroll
                                for (int r = 0; r < RMAX; r++) {
                                    const float diff = c32v[r] - s1f;
                                    near |= __builtin_amdgcn_ballot_w64(fabsf(diff) <= tolf) & live_m[r];
                                    hitr[r] = __builtin_amdgcn_ballot_w64(diff >= 0.0f) & live_m[r];
                                    anyhit |= hitr[r];
                                }
                                close = close || near != 0;
                                if (anyhit) {
                                    if (RMAX <= 4) {
                                        // the first slot that reaches s = the least of (first lane of round r) * R + r: scalar arithmetic,
                                        // no jumps (a round without a hit gives ~0u * R + r, which no real slot can exceed)
                                        unsigned int best = ~0u;
#pragma unroll
                                        for (int r = 0; r < RMAX; r++) {
                                            const unsigned int fl = hitr[r] ? (unsigned int)__builtin_ctzll(hitr[r]) : 0x0fffffffu;
                                            best = min(best, fl * (unsigned int)R_eff + (unsigned int)r);
                                        }
                                        slot_new = (int)best;
                                    } else {
                                        const int hl = (int)__builtin_ctzll(anyhit);
                                        int rr = 0;
#pragma unroll
                                        for (int r = RMAX - 1; r >= 0; r--) if ((hitr[r] >> hl) & 1ull) rr = r;
                                        slot_new = hl * R_eff + rr;
                                    }
                                } else close = true;                          // (no slot reaches s: let the fp64 path say so)
                            } else {
                                branch = 2;
                                // zero, NaN or overflowing masses: fp64 decides.  (Every comparison above is false for them, so they can only
                                // arrive here; the common branches do not pay for the test.)
                                close = close || !(totalf > 0.0f) || !(totalf < 3.0e38f);
                            }
                        }
                        need64 = close;
                        // MIX, view 0: the budget above counts roundings relative to the total, which takes fp32's NORMAL range.  Without a mix every
                        // term carries (g + beta) / den and stays there; at lambda near 1 a term is a32 * (float)mix alone, and a table may hold
                        // p_emb(w|k) of 1e-40 or 0 under every listed topic: cells, mass and root denormal or flushed, a tolerance of 2^-17 * total
                        // without meaning.  A total below 2^-100 goes to fp64 (one scalar compare, this flavour only); above it a flushed cell is
                        // wrong by less than 2^-126 * a32, a32 < 2^21: nothing beside 2^-17 * total.
                        if (MIX && mixv) need64 = need64 || !(totalf >= 0x1.0p-100f);
                    }
                    if (need64) {
#ifdef MVHDP_COUNT_SCREENED                                  /* measurement build: tokens the screening handed to fp64, reported with the exact fallbacks */
                    if (SCREEN && !exact_only) n_fb++;
#endif
                    slot_new = -1;
                    // WRK:496-513 topicDocWordMasses: terms of the lane's slots, in-lane running sum,
                    // one DPP prefix scan of the lane totals (certified below); the reference's sequential
                    // left-to-right sum only when a comparison is too close to call.
                    double cum[RMAX];
                    // MIX, view 0, under the screening: the loop carries the fp32 cells; the rare token that comes here reads its slots' fp64 cells now
                    // (the wait for them is a wait for everything in flight: in order -- once in a few thousand tokens)
                    double mg64[RMAX];
#pragma unroll
                    for (int r = 0; r < RMAX; r++) mg64[r] = (double)mg[r];
                    if (MIX && SCREEN && mixv) {
                        const gptr_t m64p = scalar_row(mix64_v, (unsigned int)w, (unsigned int)K * 8u);
#pragma unroll
                        for (int r = 0; r < RMAX; r++) mg64[r] = gather_mix<double>(m64p + ((unsigned int)koff[r] << 1));
                    }
#pragma unroll
                    for (int r = 0; r < RMAX; r++) {
                        term[r] = 0.0;
                        if (__builtin_amdgcn_inverse_ballot_w64(live_m[r])) {
                            double o = oth[r], dn = den[r];
                            if (SCREEN) slot_consts(r, o, dn);
                            double p_wt = div_inrange((double)g[r] + beta_m, dn);          // WRK:507
                            if (MIX && mixv) p_wt = mg64[r] + oml * p_wt;                  // WRK:504-505 (unfused: -ffp-contract=off)
                            term[r] = (p_mm * (double)cn[r] + o) * p_wt;                   // WRK:509
                        }
                    }
                    // u1 and tree[1] in fp64: the lane registers where the flavour keeps them; under screening the token loop carries
                    // only their fp32 roundings (four registers fewer in a kernel that spills), and the rare token that comes here
                    // draws u1 again (counter-based: the same bits) and reads tree[1] from the 8-byte-per-type root array.
                    double u1, root;
                    if (!SCREEN) { u1 = bcast_d(u1_l, TOK_T); root = bcast_d(root_l, TOK_T); }
                    else {
                        uint32_t x[4];
                        philox4x32_10((uint32_t)(c0 + TOK_T), (uint32_t)m, (uint32_t)dg, sl.sweep_idx,
                                      sl.seed_lo, sl.seed_hi ^ (uint32_t)((unsigned long long)dg >> 32), x);
                        u1 = uniform_d(bits_to_unit(x[0], x[1]));
                        root = uniform_d(mm.root[row]);
                    }
                    {
                        double lsum = term[0];
                        cum[0] = lsum;
#pragma unroll
                        for (int r = 1; r < RMAX; r++) { lsum += term[r]; cum[r] = lsum; }      // unused rounds add 0.0
                        const double incl = wave_incl_scan_d_dpp(lsum);
                        const double excl = incl - lsum;
#pragma unroll
                        for (int r = 0; r < RMAX; r++) cum[r] = (r == R_eff - 1) ? incl : excl + cum[r];
                        mass = bcast_d(incl, 63);
                    }
                    // decision on (cum, mass); tol < 0 disables the closeness checks
#define MVHDP_DECIDE(TOL)                                                                                   \
                    {                                                                                       \
                        const double tol_ = (TOL);                                                          \
                        total = newMass + mass + root;                       /* WRK:519 */                  \
                        s0 = u1 * total;                                                                    \
                        unsafe = false; slot_new = -1;                                                      \
                        if (s0 < newMass) {                                  /* WRK:522 */                  \
                            branch = 0;                                                                     \
                            unsafe = fabs(s0 - newMass) <= tol_ * total;                                    \
                        } else {                                                                            \
                            s1 = s0 - newMass;                               /* WRK:528 */                  \
                            unsafe = (newMass != 0.0 && fabs(s1) <= tol_ * total) || (fabs(s1 - mass) <= tol_ * total); \
                            if (s1 < mass) {                                 /* WRK:529 */                  \
                                branch = 1;                                                                 \
                                unsigned long long anyhit = 0, near = 0, hitr[RMAX];                        \
                                _Pragma("unroll")                                                           \
                                for (int r = 0; r < RMAX; r++) {             /* WRK:531 lower_bound over the live list */ \
                                    {                                                                       \
                                        const double diff = cum[r] - s1;     /* sign-exact: diff >= 0 <=> cum >= s1 */ \
                                        near |= __builtin_amdgcn_ballot_w64(fabs(diff) <= tol_ * total) & live_m[r]; \
                                        hitr[r] = __builtin_amdgcn_ballot_w64(diff >= 0.0) & live_m[r];     \
                                        anyhit |= hitr[r];                                                  \
                                    }                                                                       \
                                }                                                                           \
                                unsafe = unsafe || near != 0;                                               \
                                if (anyhit) {                                                               \
                                    const int hl = (int)__builtin_ctzll(anyhit);                            \
                                    int rr = 0;                                                             \
                                    _Pragma("unroll")                                                       \
                                    for (int r = RMAX - 1; r >= 0; r--) if ((hitr[r] >> hl) & 1ull) rr = r; \
                                    slot_new = hl * R_eff + rr;                                             \
                                }                                                                           \
                            } else {                                                                        \
                                branch = 2;                                                                 \
                            }                                                                               \
                        }                                                                                   \
                    }
                    // Certified scan: any summation order of the same non-negative terms differs from the
                    // sequential one by < 2n ulp-units of the total; if no comparison is closer than that the
                    // decisions equal the reference's bit for bit, otherwise the sequential sum decides.
                    MVHDP_DECIDE((double)(4 * S_used + 16) * 0x1.0p-53)
                    if (__builtin_expect(unsafe || exact_only, 0)) {
                        if (unsafe) n_fb++;
                        double c = 0.0;
                        for (int i = 0; i < S_used; i++) {                   // WRK:501-513, dense order
                            const int li = i >> lg, ri = i & (R_eff - 1);
                            double tsel = term[0];
#pragma unroll
                            for (int r = 1; r < RMAX; r++) tsel = (ri == r) ? term[r] : tsel;
                            c += bcast_d(tsel, li);
                            if (lane == li) {
#pragma unroll
                                for (int r = 0; r < RMAX; r++) if (ri == r) cum[r] = c;
                            }
                        }
                        mass = c;
                        MVHDP_DECIDE(-1.0)
                    }
#undef MVHDP_DECIDE

                    }
                    if (DEBUG) {
                        if (sl.tok_dbg[m] && lane == 0) {
                            double* gdb = sl.tok_dbg[m] + (base + c0 + TOK_T) * 4;
                            gdb[0] = newMass; gdb[1] = mass; gdb[2] = mm.root[row]; gdb[3] = s0;
                        }
                        for (int q = 0; q < sl.n_trace; q++) {
                            if (sl.trace_doc[q] == d && sl.trace_view[q] == m && sl.trace_pos[q] == c0 + TOK_T) {
                                double* out = sl.trace_out + (int64_t)q * (K + 1);
                                const double* tr = mm.trees + row * 2 * K;
                                for (int k = lane; k < K; k += WAVE) out[k] = tr[K + k] / total;
                                __threadfence();
#pragma unroll
                                for (int r = 0; r < RMAX; r++)
                                    if (r < R_eff && __builtin_amdgcn_inverse_ballot_w64(live_m[r])) out[koff[r] >> 2] += term[r] / total;
                                if (lane == 0) out[K] = newMass / total;
                                __threadfence();
                            }
                        }
                    }

                    int znew;
                    if (branch == 1) {                                       // WRK:530-531 (the common one first)
                        if (slot_new < 0) {                                  // lower_bound == -1 -> exception, Q11: the entity is abandoned.
                            aborted = true;                                  // As data, not as a way out of the loop (a second exit costs every
                            n_tok -= (unsigned int)__popcll(rem);            // token scalar bookkeeping): no token is left to visit (the chunk's
                            rem = 0;                                         // were counted up front), and this one keeps its topic
                            znew = bcast_i(z_l, TOK_T);
                        } else {
                            const int rn = slot_new & (R_eff - 1), ln = slot_new >> lg;
                            int ksel = koff[0];
#pragma unroll
                            for (int r = 1; r < RMAX; r++) ksel = (rn == r) ? koff[r] : ksel;
                            znew = bcast_i(ksel, ln) >> 2;
                        }
                    } else if (branch == 0) {                                // WRK:523-526
                        c_new++;
                        znew = mm.first_inactive;
                        if (sl.births) {                                     // the first topic no delta has reached yet (the updater of the reference removes a
                            const int bp_ = __hip_atomic_load(&sl.births[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // topic from inActiveTopicIndex with the first delta)
                            znew = bp_ < sl.births[1] ? sl.births[2 + bp_] : -1;
                        }
                        if (znew < 0) znew = K - 1;                          // WRK:549-552
                        const uint32_t wbit = bitmap[znew >> 5];
                        slot_new = ((wbit >> (znew & 31)) & 1u) ? (int)(prefix[znew >> 5] + __popc(wbit & ((1u << (znew & 31)) - 1u))) : -1;
                        slot_new = uniform_i(slot_new);
                    } else {                                                 // WRK:533-535
                        c_tree++;
                        if (WALK) whist_l += (lane == min((int)(bcast_f(u1f_l, TOK_T) * MVHDP_WALK_BINS), MVHDP_WALK_BINS - 1)) ? 1u : 0u;   // lane b counts bin b of u1
                        if (!WALK || ((walked >> TOK_T) & 1ull)) {
                            znew = bcast_i(zt_l, TOK_T);
                            slot_new = bcast_i(st_l, TOK_T);
                        } else if (LIVEROWS && !(NARROW && (wfull_t & W_HEAVY))) {   // the word's LIVE row (UPD:242-260 keeps the reference's leaves current)
                            n_od++;
                            unsigned long long t_rs1 = 0;
#ifdef MVHDP_TIMING
                            const unsigned long long t_rs0 = __builtin_amdgcn_s_memtime();
#endif
                            if (sl.flags & MVHDP_SL_NO_ROW_SAMPLE) znew = bcast_i(z_l, TOK_T);      // (measurement only, MVHDP_NO_ROW_SAMPLE)
                            else
                            znew = uniform_i(row_sample_live<(NARROW != 0), LIVEROWS == 2>(rowq, spec_t, coef_s != nullptr, (const __attribute__((address_space(3))) float*)coef_s + m * Kp, mm.coef + (int64_t)m * Kp, smp_m, smS, rowp_t, K,
                                                                     bcast_f(u2f_l, TOK_T), bcast_f(root32_l, TOK_T), bsel_t, (LIVEROWS == 2 && bsel_t) ? mm.mass0[row] : 0.0f /* (a scalar load: the address is wave-uniform) */, lane, &t_rs1));
                            if (znew < 0) znew = K - 1;                      // WRK:549-552
#ifdef MVHDP_TIMING
                            t_rows += __builtin_amdgcn_s_memtime() - t_rs0;
                            if (t_rs1) t_rows_wait += t_rs1 - t_rs0;
#endif
                            const uint32_t wbit = bitmap[znew >> 5];
                            slot_new = ((wbit >> (znew & 31)) & 1u) ? (int)(prefix[znew >> 5] + __popc(wbit & ((1u << (znew & 31)) - 1u))) : -1;
                            slot_new = uniform_i(slot_new);
                        } else {                                             // not walked at the chunk head: FT:118-132 now
                            n_od++;
                            uint32_t x[4];
                            philox4x32_10((uint32_t)(c0 + TOK_T), (uint32_t)m, (uint32_t)dg, sl.sweep_idx,
                                          sl.seed_lo, sl.seed_hi ^ (uint32_t)((unsigned long long)dg >> 32), x);
                            znew = uniform_i(dtab_sample_uniform(mm, row, bits_to_unit(x[2], x[3])));
                            // (live-rows form, a heavy word: a leaf that is zero whatever the counts cannot come from a tree read whole -- see the
                            // chunk head; the token then takes its topic from the smoothing parts alone, which heavy_refresh_kernel does not touch)
                            if (LIVEROWS && NARROW && !(mm.coef[(int64_t)m * Kp + znew] > 0.0f))
                                znew = uniform_i(smoothing_sample_live(smp_m, K, (float)bits_to_unit(x[2], x[3]) * smS, lane));
                            const uint32_t wbit = bitmap[znew >> 5];
                            slot_new = ((wbit >> (znew & 31)) & 1u) ? (int)(prefix[znew >> 5] + __popc(wbit & ((1u << (znew & 31)) - 1u))) : -1;
                            slot_new = uniform_i(slot_new);
                        }
                        if (znew < 0) znew = K - 1;                          // WRK:549-552
                    }
                    znew = uniform_i(znew);

                    // WRK:557-560
                    znew_l = wave_writelane(znew_l, znew, TOK_T);
                    if (slot_new >= 0) {
                        const int rn = slot_new & (R_eff - 1), ln = slot_new >> lg;
#pragma unroll
                        for (int r = 0; r < RMAX; r++) if (rn == r) cn[r] = wave_writelane(cn[r], bcast_i(cn[r], ln) + 1, ln);
                    }
}
