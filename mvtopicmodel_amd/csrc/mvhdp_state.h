// mvhdp_state.h — what the device buffers of one handle currently hold (mvhdp_ctx::st), kept in one place: the fields are private, they
// are read through the accessors and written ONLY by the transitions below, each of which records one event that happened to the
// buffers.  The host-side sources (mvhdp_api.hip, mvhdp_enqueue.hip, mvhdp_group.hip, mvhdp_emb.hip, mvhdp_diag.hip, mvhdp_remap.hip, mvhdp_split.hip) call these and
// nothing else; tests/test_handle_state.py compiles this file with the host compiler: no HIP type in here.
//
// The rules the callers keep with it:
//   - stale trees are never sampled from: REUSE_TREES / FROZEN ask trees_current(), every other sweep builds its own;
//   - pending deltas are never applied twice or recounted on top: a sampling sweep is refused while delta_pending(), a recount drops them;
//   - leftovers in the 16-bit delta cells are put back to the bias before the cells are used again (delta16_used()).
//
// Which event leaves which field how ("." = as it was).  C = have_counts, S = counts_stale, T = have_trees, F = full_trees,
// I = trees_inference, L = last_need_full, Z = delta_clean, P = delta_pending, H = delta16_used, O = deltas_dirty, R = rows_applied,
// N = nslots_valid, U = unassigned (per view).
//
//   transition                         C S T F I L Z P H O R   N U
//   corpus_replaced(m, any)            0 . 0 . . . . . . . .   0 U[m] = any
//   assignments_replaced(m, any)       . * . . . . . . . . .   0 U[m] = any (m < 0: every view)      * S = 1 if C
//   every_token_assigned()             . . . . . . . . . . .   . every view 0
//   counts_rebuilt()                   1 0 0 . . . . . . . .   . .
//   counts_went_stale()                . 1 . . . . . . . . .   . .
//   trees_built(full, inference)       . . 1 f i . . . . . .   . .
//   full_trees_written()               . . . 1 . . . . . . .   . .
//   trees_outdated()                   . . 0 . . . . . . . .   . .
//   trees_overwritten()                . . 0 0 . . . . . . .   . .
//   sweep_planned(need_full)           . . . . . n . . . . .   . .
//   delta_zeroed()                     . . . . . . 1 0 . . .   . .
//   delta_written(in16)                . . . . . . 0 . * . .   . .                                   * H = 1 if in16
//   delta_left_pending()               . . . . . . . 1 . . .   . .
//   delta_applied()                    . . 0 . . . 1 0 . . .   . .     = delta_zeroed + trees_outdated
//   delta_discarded(overwritten)       . 1 . . . . * 0 . . .   . .                                   * Z = 0 if overwritten
//   delta16_rebiased()                 . . . . . . . . 0 . .   . .
//   overlap_enqueued() / _finished()   . . . . . . . . . 1/0 . . .
//   bracket_begun()                    . . 0 . . . . . . . 0   . .
//   bracket_rows(n)                    . . . . . . . . . . +n  . .
//   bracket_closed(nrows)              . . . . . . . . . . -1  . .     returns R == nrows (before)
//   bracket_abandoned()                . . 0 . . . . . . . -1  . .
//   nslots_counted(valid)              . . . . . . . . . . .   v .
//   nslots_invalidated()               . . . . . . . . . . .   0 .
//
// What a caller can observe after each kind of sweep follows from these: profiles/enqueue_refactor.md has that table, and
// profiles/handle_state.md maps every call site to its transition.
//
// Invariants.  The transitions are the parent sites' writes and nothing more, so taken in ANY order they reach every combination of the
// fields (tests/test_handle_state.py walks the closure); what holds, holds through the order the callers keep:
//   (a) delta_pending implies !delta_clean -- on every path of the library: delta_left_pending() is the finish of a NO_APPLY sweep whose
//       enqueue called delta_written(), and nothing between the two halves touches the handle.  Freely: delta_zeroed, delta_left_pending.
//   (b) an open bracket implies !have_trees -- NOT held by the ABI: mvhdp_apply_delta_begin, then mvhdp_build_trees (which does not ask
//       bracket_open()) leaves both; mvhdp_apply_delta_end then overwrites the flag.  Freely: bracket_begun, trees_built.
//   (c) delta16_used implies !delta_clean -- held except behind a double failure: a deferred sweep on the 16-bit cells that fails before
//       its apply pass, then mvhdp_group_build_counts whose member recount fails before it re-biases: the group zeroes the 32-bit buffer
//       (delta_zeroed) and the cells keep their leftovers.  Freely: delta_written(true), delta_zeroed.
// While have_trees is false, full_trees and trees_inference describe the LAST build: trees_outdated() leaves them, the arrays still hold
// that build and only its inputs moved on.  Nothing acts on them in that state: ensure_full_trees returns before reading either unless
// trees_current(); the sweep-start upgrade of mvhdp_enqueue.hip (need_full && !full_trees()) runs behind trees_built() of the same
// function or on the trees REUSE_TREES was checked for, and behind trees_overwritten() only with need_full false (a live-rows plan
// never needs FTree.tree, mvhdp_plan.h) -- there it reads full_trees() without current trees, as intended, and goes no further.
#pragma once
#include <cstdint>

class ModelState {
    bool have_counts_ = false, counts_stale_ = false;
    bool have_trees_ = false, full_trees_ = false, trees_inference_ = false, last_need_full_ = true;
    bool delta_clean_ = false, delta_pending_ = false, delta16_used_ = false, deltas_dirty_ = false;
    int64_t rows_applied_ = -1;
    bool nslots_valid_ = false;
    uint32_t unassigned_ = 0;                // bit m: some token of view m may still carry UNASSIGNED_TOPIC (-1, PTM:63)
    friend struct ModelStateProbe;           // defined by the CPU test's shim alone: sets up a starting state, reads the fields back

public:
    bool have_counts() const { return have_counts_; }        // the count table was built or supplied for this corpus
    bool counts_stale() const { return counts_stale_; }      // the assignments moved without the counts: a sampling sweep is refused
    bool trees_current() const { return have_trees_; }       // the descent table is that of the current counts, hyper-parameters and mix
    bool full_trees() const { return full_trees_; }          // the last build wrote the FTree.tree arrays too (a sweep may refresh only the descent table)
    bool trees_inference() const { return trees_inference_; }   // leaves of the last build: p_wt alone (INF:576)
    bool last_need_full() const { return last_need_full_; }  // the last sweep's kernels could reach the generic kernel (needs FTree.tree itself)
    bool delta_clean() const { return delta_clean_; }        // the delta buffer is known to be all zero
    bool delta_pending() const { return delta_pending_; }    // a NO_APPLY sweep has left deltas that nothing has consumed yet
    bool delta16_used() const { return delta16_used_; }      // MvModel::delta16 holds deltas of the last sweep (until the apply pass)
    bool deltas_dirty() const { return deltas_dirty_; }      // an overlapped segmented sweep was enqueued and not seen to finish: delta2 / delta3 may hold leftovers
    bool bracket_open() const { return rows_applied_ >= 0; } // between mvhdp_apply_delta_begin and _end
    bool nslots_valid() const { return nslots_valid_; }      // MvModel::nslots and the two histograms describe the current assignments
    // A live sweep on the 16-bit mirror needs every row's total to be constant; a first visit of an unassigned token only adds to its
    // row, so while this holds live sweeps stay on the 32-bit table.
    bool any_unassigned() const { return unassigned_ != 0; }
    bool view_unassigned(int m) const { return (unassigned_ >> m & 1u) != 0; }   // the same of view m alone

    // mvhdp_set_corpus: view m has new tokens, all unassigned (if it has any); the counts and trees of the old corpus mean nothing
    void corpus_replaced(int m, bool any_tokens) { set_unassigned(m, any_tokens); nslots_valid_ = false; have_counts_ = false; have_trees_ = false; }
    // z of view m (m < 0: of every view, none left unassigned) was written from outside the sweep: counts that exist no longer describe it
    void assignments_replaced(int m, bool any_unassigned)
    {
        if (m < 0) unassigned_ = 0; else set_unassigned(m, any_unassigned);
        nslots_valid_ = false;
        if (have_counts_) counts_stale_ = true;
    }
    // a sampling sweep visited every entity and abandoned none (WRK:557)
    void every_token_assigned() { unassigned_ = 0; }
    // the counts are those of z again: recounted, supplied by the host, or written by it in place
    void counts_rebuilt() { have_counts_ = true; have_trees_ = false; counts_stale_ = false; }
    // z moved on (or an exchange broke) and the counts did not follow: a recount is due
    void counts_went_stale() { counts_stale_ = true; }
    // a build pass over every row was enqueued from the current counts
    void trees_built(bool full, bool inference) { have_trees_ = true; full_trees_ = full; trees_inference_ = inference; }
    // the FTree.tree arrays were written behind a build that had left them out
    void full_trees_written() { full_trees_ = true; }
    // what the trees were built from has changed: counts, alpha, the hyper-parameters or the mix
    void trees_outdated() { have_trees_ = false; }
    // the live-rows form wrote its coefficients where the stored trees were
    void trees_overwritten() { have_trees_ = false; full_trees_ = false; }
    // a sweep's plan is about to be enqueued
    void sweep_planned(bool need_full) { last_need_full_ = need_full; }
    // the delta buffer was cleared, or a pass that zeroes what it adds went over all of it; nothing in it waits to be applied
    void delta_zeroed() { delta_clean_ = true; delta_pending_ = false; }
    // a sweep's atomics (or the after - before pass of a live NO_APPLY sweep) go to the delta buffer; in16: to the 16-bit cells as well
    void delta_written(bool in16) { delta_clean_ = false; if (in16) delta16_used_ = true; }
    // a NO_APPLY sweep finished: its deltas wait for mvhdp_apply_delta / the bracket / a recount
    void delta_left_pending() { delta_pending_ = true; }
    // the deltas went into the counts and the buffer is zero again
    void delta_applied() { delta_zeroed(); trees_outdated(); }
    // a group's step failed: the deltas will never be applied; overwritten: the collective left other ranks' sums in the buffer
    void delta_discarded(bool overwritten) { delta_pending_ = false; counts_stale_ = true; if (overwritten) delta_clean_ = false; }
    // the 16-bit delta cells are back at the bias (folded in by the apply pass, or reset)
    void delta16_rebiased() { delta16_used_ = false; }
    // overlapped segments: delta2 / delta3 are in use; the sweep was seen to finish, its apply passes left them zero
    void overlap_enqueued() { deltas_dirty_ = true; }
    void overlap_finished() { deltas_dirty_ = false; }
    // mvhdp_apply_delta_begin / _rows / _end; closed: whether the ranges covered nrows rows (exactly once is the caller's promise)
    void bracket_begun() { rows_applied_ = 0; have_trees_ = false; }
    void bracket_rows(int64_t n) { rows_applied_ += n; }
    bool bracket_closed(int64_t nrows) { const bool exact = rows_applied_ == nrows; rows_applied_ = -1; return exact; }
    // a bracket that will not be closed (a group's step failed): rows were applied under trees that are now half rebuilt
    void bracket_abandoned() { rows_applied_ = -1; have_trees_ = false; }
    // MvModel::nslots was recounted from z or left by a sweep (valid: no entity was abandoned); or can no longer be trusted
    void nslots_counted(bool valid) { nslots_valid_ = valid; }
    void nslots_invalidated() { nslots_valid_ = false; }

private:
    void set_unassigned(int m, bool v) { unassigned_ = v ? unassigned_ | (1u << m) : unassigned_ & ~(1u << m); }
};
