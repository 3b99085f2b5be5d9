"""Near-ties of the sweep's decisions under the useVectorsLambda mix, constructed with the sequential restatement alone
(tests/mix_ref.py; no GPU, no product code), the way tests/near_ties.py constructs them under hyper-parameters with the oracle.

The outcome of one deferred sweep is a piecewise constant function of lambda, and of any single cell of expDotProductValues.
Bisecting an interval whose ends give different assignments down to ADJACENT doubles yields a flip: two values one ulp apart between
which a comparison of some view-0 token changes sides (lambda reaches the view-0 document terms and the view-0 leaves only, so the
first token that differs is a view-0 token).  tests/near_ties.py's bisect / classify / find_flips / ladder work on any evaluator with
Evaluator's interface; MixEvaluator is one, with the parameters

    ("lam",)          lambda itself, inside (0, 1)
    ("cell", k, w)    expDotProductValues[k][w] (sumExpValues held fixed)
"""
import numpy as np

from tests import near_ties
from tests.mix_cases import set_hyper_o, table
from tests.mix_ref import MixRef


class MixEvaluator:
    live = None                                        # (deferred sweeps only: the restatement has no live form)
    plant = 0

    def __init__(self, case, seed, lam, table_seed=3, sweep_idx=0):
        self.case, self.seed, self.sweep_idx, self.lam = case, int(seed), int(sweep_idx), float(lam)
        self.e, self.S = table(case.K, case.V[0], table_seed)
        self.o = MixRef(case.K, case.V)
        for m in range(case.M):
            self.o.set_corpus(m, case.doc_off[m], case.tokens[m])
        set_hyper_o(self.o, case.hy)
        self.order = np.arange(case.D, dtype=np.int64)
        self.rank = self.order.copy()
        self.n_eval = 0

    def mix_at(self, param, x):
        """(lambda, expDot, sumExp) with the parameter at x"""
        if param[0] == "lam":
            return float(x), self.e, self.S
        if param[0] == "cell":
            e = self.e.copy()
            e[param[1], param[2]] = x
            return self.lam, e, self.S
        raise ValueError(param)

    def hyper_at(self, param, x):
        return self.case.hy

    def prepare(self, model, param, x):
        """bring the restatement or a sampler to the state before the sweep (the hyper-parameters are set once: they do not move)"""
        for m in range(self.case.M):
            model.set_assignments(m, self.case.z0[m])
        model.build_counts()
        model.set_vectors_mix(*self.mix_at(param, x))

    def run(self, param, x, want_dbg=False):
        o = self.o
        set_hyper_o(o, self.case.hy)                   # (an activation of the last sweep moved alpha and the inactive set)
        self.prepare(o, param, x)
        self.n_eval += 1
        r = o.sweep(self.sweep_idx, self.seed, want_dbg=want_dbg)
        return near_ties.Outcome([o.get_assignments(m) for m in range(self.case.M)], r["stats"], r.get("dbg"))


def searches(case, lam, n=14):
    """aimed searches for the two rare comparisons, then plain ones: lambda in short intervals above `lam`, and single cells of the
    table under frequent view-0 types"""
    out = []
    # aimed at the first token of every entity (near_ties.Search): lambda over nearly its whole range moves that token's document term
    # against its tree's root and the new-topic mass; bisection needs no monotony, only ends that differ
    for r in range(-(-40 // case.D)):                  # (every seed draws other uniforms: some first token's lies where the branch changes hands)
        out.append(near_ties.Search(("lam",), 0.03125, 0.96875, "B", 20 + r))
    for r in range(2):
        out.append(near_ties.Search(("lam",), 0.03125, 0.96875, "A", 40 + r))
    for r in range(n):
        x0 = lam * (1.0 + 0.03125 * r)
        out.append(near_ties.Search(("lam",), x0, min(x0 * (1.0 + 2.0 ** -5), 1.0), "any", 60 + r))
    freq = np.argsort(-np.bincount(case.tokens[0][case.tokens[0] < case.V[0]], minlength=case.V[0]), kind="stable")
    rng = np.random.RandomState(2)
    for r in range(n):
        w, k = int(freq[r % 4]), int(rng.randint(0, case.K))
        out.append(near_ties.Search(("cell", k, w), 0.25, 1.0, "any", 90 + r))
    return out


CAP = {"A": 3, "B": 4, "C": 6, "D": 2}
# the rungs of a ladder: the flip's ends, every tolerance a sampler decides by (the certified scan's about 2^6..2^12 ulp, the screen's
# 2^-17 relative = 2^36 ulp), and far outside
JS = [0, 2, 4, 6, 8, 10, 12, 16, 24, 32, 36, 38, near_ties.J_MAX]
# case -> (constructor, forced register variants that serve every entity of it, lambda, the kinds its fixed searches must yield).
# lambda moves a view-0 token's document term and its tree's root together, so a flip of the count / tree comparison (kind B, WRK:529) is
# rare: the two cases with ten and six entities yield one, the cases of two to four long entities yield slot boundaries (kind C,
# WRK:531: hundreds per token) and, below K = 1000, the new-topic comparison (kind A, WRK:522).
PLAN = {"small": (near_ties.case_small, [1], 0.25, "ABC"), "mid2": (near_ties.case_mid2, [2], 0.4, "ABC"), "mid4": (near_ties.case_mid4, [4], 0.25, "AC"),
        "wide8": (near_ties.case_wide8, [8], 0.25, "C"), "wide16": (near_ties.case_wide16, [16], 0.6, "C")}


def flips_of(name):
    make, forced, lam, _ = PLAN[name]
    case = make()
    ev = MixEvaluator(case, 5, lam)
    return ev, near_ties.find_flips(ev, searches(case, lam), CAP), forced


def ladder_kept(ev, flip, js=JS):
    """(rungs the restatement kept, rungs it abandoned an entity at)"""
    dropped = [0]
    kept = sum(1 for _ in near_ties.ladder(ev, flip, js, dropped))
    return kept, dropped[0]


def check_quotas(name, flips):
    """what a case must give before its ladders mean anything: comparisons against the document-term sums among the flips"""
    n = {k: sum(f.kind == k for f in flips) for k in "ABCD"}
    assert n["A"] + n["B"] + n["C"] >= 6 and n["C"] >= 2 and all(n[k] >= 1 for k in PLAN[name][3]), n
