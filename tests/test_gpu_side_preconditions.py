"""What the side calls on a trained handle answer when the handle is not in the state they need, and which of two faults a doubly-wrong
call reports: the return code of every entry and the start of its message, on one tiny model (M = 2, K = 4, V = [6, 5], D = 8).  The
checks, the call prologue and the timer behind these entries are shared (mvtopicmodel_amd/csrc/mvhdp_side.h); this pins what a caller
can observe of them.  Every expectation is what this very table returned on an MI355X against the library of the commit before the
shared header existed (deb7db7), not reasoned out from the code under test; message parts are cut where the wordings were unified."""
import numpy as np
import pytest

from mvtopicmodel_amd import NativeSampler
from mvtopicmodel_amd._lib import MvhdpError
from mvtopicmodel_amd.native import Hyper, SWEEP_NO_APPLY
from tests.helpers import make_native, make_oracle, small_corpus

pytestmark = pytest.mark.gpu

OK, INV, STATE = 0, -1, -2
K, V, D = 4, [6, 5], 8
W = np.array([1.0, 1.0])
ZERO = np.array([0.0, 0.0])
NEW_OFF = np.array([0, 3, 5], dtype=np.int64)                  # two unseen documents of view 0
NEW_TOK = np.array([1, 5, 2, 0, 3], dtype=np.int32)
BAD_TOK = np.array([1, -2, 2, 0, 3], dtype=np.int32)
OFF_FROM_1 = np.array([1, 3, 5], dtype=np.int64)
COHORTS = [[0, 1], [2]]


def _model():
    c = small_corpus(K, V, D, [5, 4], 17)
    hy = Hyper.defaults(K, V)
    o = make_oracle(c, hy)
    return c, hy, [o.get_assignments(m) for m in range(c.M)]


def _handle(model, state):
    c, hy, z = model
    if state in ("no hyper, no counts", "no hyper"):
        s = NativeSampler(c.K, c.V, device=0)
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m])
            s.set_assignments(m, z[m])
        if state == "no hyper":
            s.build_counts()
        return s
    s = make_native(c, hy, z)
    if state == "stale":                                       # assignments set after the counts
        s.set_assignments(0, z[0])
    elif state == "pending":                                   # a NO_APPLY sweep's deltas wait beside the counts
        s.sweep(0, 5, flags=SWEEP_NO_APPLY)
    else:
        assert state == "current"
    return s


# ---- one minimal call per entry; kw overrides make it wrong in a second way ----
def top_words(s, m=0, n=2):
    return s.top_words(m, n)


def diagnostics(s, n=2):
    return s.diagnostics(num_top_words=n)


def predict_items(s, m=0, w=W, n=2, d0=0):
    return s.predict_items(m, w, n, d0=d0)


def score_items(s, m=0, w=W, d0=0):
    return s.score_items(m, w, [1], [1], d0=d0)


def predict_entities(s, m=0, w=W, n=2, c0=0):
    return s.predict_entities(m, w, n, items=[[1]], c0=c0)


def rank_entities(s, m=0, w=W, c0=0):
    return s.rank_entities(m, w, [0], [1], items=[[1]], c0=c0)


def gram_words(s, m=0, r1=None):
    return s.topic_gram("words", m=m, r1=V[0] if r1 is None else r1)


def gram_entities(s, w=W, r0=0):
    return s.topic_gram("entities", view_weights=w, r0=r0)


def cohort_share(s, m=0, n=2, cohorts=COHORTS):
    return s.cohort_top_words(m, cohorts, n=n, order="share")


def cohort_count(s):
    return s.cohort_top_words(0, COHORTS, n=2, order="count")


def heldout(s, m=0, particles=2, off=NEW_OFF, tok=NEW_TOK):
    return s.heldout_left_to_right(off, tok, particles=particles, seed=3, m=m)


def fold_in(s, w=W, iterations=2, tok=NEW_TOK, coupling=None):
    return s.fold_in([NEW_OFF, None], [tok, None], w, iterations=iterations, seed=3, coupling=coupling)


NEED_CURRENT = [top_words, diagnostics, predict_items, score_items, predict_entities, rank_entities, gram_words, cohort_share]
AS_THEY_ARE = [cohort_count, heldout, fold_in]                 # documented to take the counts as the handle holds them

# (state, call, overrides, code, part of the message)
ROWS = (
    [("stale", f, {}, STATE, "") for f in NEED_CURRENT] +
    [("pending", f, {}, STATE, "pending") for f in NEED_CURRENT] +
    [("no hyper, no counts", f, {}, STATE, "") for f in NEED_CURRENT] +
    [(st, f, {}, OK, "") for st in ("stale", "pending") for f in AS_THEY_ARE] +
    [
        # set_hyper is asked for before the counts, where an entry needs it at all
        ("no hyper", top_words, {}, OK, ""),
        ("no hyper", cohort_share, {}, OK, ""),
        ("no hyper", diagnostics, {}, STATE, "diagnostics before set_hyper"),
        ("no hyper", predict_items, {}, STATE, "predict_items before set_hyper"),
        ("no hyper", score_items, {}, STATE, "score_items before set_hyper"),
        ("no hyper", predict_entities, {}, STATE, "predict_entities before set_hyper"),
        ("no hyper", rank_entities, {}, STATE, "rank_entities before set_hyper"),
        ("no hyper", gram_words, {}, STATE, "topic_gram before set_hyper"),
        ("no hyper", heldout, {}, STATE, "heldout_left_to_right before set_hyper"),
        ("no hyper", fold_in, {}, STATE, "fold_in before set_hyper"),
        # ---- two faults at once: which one is reported ----
        ("stale", top_words, dict(m=7), INV, "top_words: bad view"),
        ("pending", top_words, dict(n=65), INV, "top_words: n must be 1..64"),
        ("stale", diagnostics, dict(n=0), INV, "diagnostics: num_top_words must be 1..64"),
        ("stale", predict_items, dict(m=2), INV, "predict_items: bad view"),
        ("stale", predict_items, dict(d0=-1), STATE, "predict_items: the counts are not current"),
        ("pending", score_items, dict(d0=-1), STATE, "score_items: a NO_APPLY sweep's deltas are pending"),
        ("current", score_items, dict(w=ZERO, d0=-1), INV, "score_items: bad entity range"),
        ("current", predict_items, dict(w=ZERO, n=0), INV, "predict_items: the view weights do not sum to a positive"),
        ("pending", predict_entities, dict(m=-1), INV, "predict_entities: bad view"),
        ("stale", rank_entities, dict(c0=-1), STATE, "rank_entities: the counts are not current"),
        ("current", predict_entities, dict(w=ZERO, n=0), INV, "predict_entities: the view weights do not sum to a positive"),
        ("current", predict_entities, dict(w=ZERO, c0=-1), INV, "predict_entities: bad candidate range"),
        ("current", predict_entities, dict(n=1025, c0=D + 1), INV, "predict_entities: bad candidate range"),
        ("stale", gram_words, dict(m=5), INV, "topic_gram: bad view"),
        ("stale", gram_words, dict(r1=V[0] + 1), STATE, "topic_gram: the counts are not current"),
        ("current", gram_entities, dict(w=ZERO, r0=-1), INV, "topic_gram: bad entity range"),
        ("current", gram_entities, dict(w=np.array([1.0, -1.0])), INV, "topic_gram: a view weight is negative or not finite"),
        ("stale", cohort_share, dict(m=9), INV, "cohort_top_words: bad view"),
        ("stale", cohort_share, dict(cohorts=[[0, D]]), STATE, "cohort_top_words: BY_SHARE"),
        ("pending", cohort_share, dict(n=0), INV, "cohort_top_words: n must be 1..64"),
        ("pending", cohort_share, dict(cohorts=(np.array([1, 1]), np.array([0]))), INV, "cohort_top_words: member_off"),
        ("current", heldout, dict(m=3, particles=0), INV, "heldout_left_to_right: bad view"),
        ("current", heldout, dict(particles=0, tok=BAD_TOK), INV, "heldout_left_to_right: particles"),
        ("current", heldout, dict(off=OFF_FROM_1, tok=BAD_TOK), INV, "heldout_left_to_right: doc_off"),
        ("no hyper, no counts", heldout, dict(tok=BAD_TOK), INV, "heldout_left_to_right: negative token"),
        ("current", fold_in, dict(iterations=0, coupling=-np.ones((2, 2))), INV, "fold_in: iterations"),
        ("current", fold_in, dict(coupling=-np.ones((2, 2)), w=ZERO), INV, "fold_in: a coupling entry is negative or not finite"),
        ("current", fold_in, dict(w=ZERO, tok=BAD_TOK), INV, "fold_in: the view weights"),
        ("no hyper, no counts", fold_in, dict(tok=BAD_TOK), INV, "fold_in: negative token"),
    ])


def test_codes_and_messages_of_every_side_entry_in_every_handle_state():
    model = _model()
    handles = {}
    got = []
    for state, call, kw, code, part in ROWS:
        if state not in handles:
            handles[state] = _handle(model, state)
        rc, msg = OK, ""
        try:
            call(handles[state], **kw)
        except MvhdpError as e:
            rc, msg = e.code, str(e)
        what = f"{state}: {call.__name__}({', '.join(kw)})"
        print(f"{what} -> {rc} {msg!r}")
        got.append((what, rc, msg, code, part))
    for s in handles.values():
        s.close()

    def as_expected(rc, msg, code, part):                      # "pending": anywhere in the message; every other part: how the message starts
        if rc != code:
            return False
        return part in msg if part in ("", "pending") else msg.startswith(f"mvhdp error {rc}: {part}")

    wrong = [f"{what}: {rc} {msg!r}, expected {code} with {part!r}" for what, rc, msg, code, part in got if not as_expected(rc, msg, code, part)]
    assert not wrong, "\n".join(wrong)


def test_every_timed_side_call_reports_a_positive_kernel_time():
    """One call of each entry that times its kernels, on the tiny model with current counts: kernel_ms is reported and positive."""
    s = _handle(_model(), "current")
    times = {
        "predict_entities": predict_entities(s).stats.kernel_ms,
        "topic_gram": gram_words(s).stats.kernel_ms,
        "cohort_top_words": cohort_share(s).stats.kernel_ms,
        "fold_in": fold_in(s).kernel_ms,
    }
    s.close()
    print("kernel_ms:", times)
    assert all(np.isfinite(t) and t > 0.0 for t in times.values()), times
