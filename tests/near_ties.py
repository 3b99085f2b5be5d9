"""Near-ties of the sweep's sampling decisions, constructed with the CPU oracle alone (no GPU, no product code).

Every integer a sweep produces comes from three comparisons per token -- s < newMass (WRK:522), s < mass (WRK:529),
cum_i >= s (WRK:531) -- and, in the tree branch, the comparisons of the F+tree descent (FT:118-132).  The draws are
counter-based and the oracle is deterministic, so the outcome of one sweep is a piecewise constant function of any
scalar hyper-parameter.  Bisecting an interval whose ends give different outcomes down to ADJACENT doubles yields a
*flip*: two parameter values one ulp apart between which some comparison changes sides, so its operands differ by a
few fp64 ulps of the total mass there.  A *ladder* walks away from the flip in powers of two of that ulp and so moves
the comparison's margin through every tolerance a sampler may use to decide the comparison in lower precision or in
another summation order.

    ev    = Evaluator(case, seed)                  # or Evaluator(case, seed, live=dict(rows=1, cell16=0))
    flips = find_flips(ev, searches_deferred(case), DEFERRED_CAP)    # the fixed lists the GPU tests use; deterministic
    for rung in ladder(ev, flip): ...              # ev.o holds the oracle's state after the sweep at rung.x

Parameters are named ("gamma", m), ("alpha", m, k) (k = K: the new-topic weight; alpha_sum is held fixed) and
("beta", m) (beta_sum is held fixed).
"""
from dataclasses import dataclass, field

import numpy as np

from oracle.binding import Oracle

WAVE = 64


# ---------------------------------------------------------------------------------------------------------------------
# cases: a corpus, initial assignments and hyper-parameters
@dataclass
class Hyp:
    """The hyper-parameters oracle and sampler read (the fields of mvtopicmodel_amd.native.Hyper)."""
    alpha: np.ndarray
    alpha_sum: np.ndarray
    beta: np.ndarray
    beta_sum: np.ndarray
    gamma: np.ndarray
    p_a: np.ndarray
    p_b: np.ndarray
    inactive: np.ndarray = None

    def copy(self):
        return Hyp(*[None if a is None else np.array(a, copy=True) for a in
                     (self.alpha, self.alpha_sum, self.beta, self.beta_sum, self.gamma, self.p_a, self.p_b, self.inactive)])


def hyper(K, V, alpha=0.1, beta=0.01, gamma=1.0, p_a=0.31, p_b=1.0, inactive=None, alpha_new=None):
    M = len(V)
    a = np.full((M, K + 1), float(alpha), dtype=np.float64)
    if alpha_new is not None:
        a[:, K] = alpha_new
    return Hyp(alpha=a, alpha_sum=np.full(M, K * float(alpha)), beta=np.full(M, float(beta)),
               beta_sum=np.array([float(beta) * v for v in V]), gamma=np.full(M, float(gamma)),
               p_a=np.full((M, M), float(p_a)), p_b=np.full((M, M), float(p_b)),
               inactive=None if inactive is None else np.asarray(inactive, dtype=np.uint8))


@dataclass
class Case:
    name: str
    K: int
    V: list
    doc_off: list
    tokens: list
    z0: list
    hy: Hyp

    @property
    def M(self):
        return len(self.V)

    @property
    def D(self):
        return len(self.doc_off[0]) - 1

    @property
    def total_tokens(self):
        return int(sum(int(o[-1]) for o in self.doc_off))

    def list_lengths(self):
        """the length of every entity's topic list (S_used of the register kernels: topics with a token in any view)"""
        return [len(np.unique(np.concatenate([self.z0[m][self.doc_off[m][d]:self.doc_off[m][d + 1]] for m in range(self.M)])))
                for d in range(self.D)]

    def max_list(self):
        return max(self.list_lengths())


def make_case(name, K, V, lens, seed, topics_per_entity, n_inactive=0, **hy_kw):
    """lens[m] = token counts of the entities in view m.  Every entity draws its initial topics from a random set of
    `topics_per_entity` (one number, or one per entity) active topics, which bounds the length of its topic list."""
    rng = np.random.RandomState(seed)
    M, D = len(V), len(lens[0])
    inactive = None
    active = np.arange(K)
    if n_inactive:
        inactive = np.zeros(K, dtype=np.uint8)
        inactive[rng.choice(K, size=n_inactive, replace=False)] = 1
        active = np.flatnonzero(inactive == 0)
    per = topics_per_entity if np.ndim(topics_per_entity) else [topics_per_entity] * D
    sets = [rng.choice(active, size=min(int(per[d]), len(active)), replace=False) for d in range(D)]
    offs, toks, z0 = [], [], []
    for m in range(M):
        L = np.asarray(lens[m], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        # a skewed type distribution: some cells of n_wk hold many tokens, most hold none
        w = rng.dirichlet(np.full(V[m], 0.3))
        toks.append(rng.choice(V[m], size=int(off[-1]), p=w).astype(np.int32))
        z0.append(np.concatenate([rng.choice(sets[d], size=int(L[d])) for d in range(D)] + [np.zeros(0, dtype=np.int64)]).astype(np.int32))
        offs.append(off)
    return Case(name, K, list(V), offs, toks, z0, hyper(K, V, inactive=inactive, **hy_kw))


# ---------------------------------------------------------------------------------------------------------------------
# parameters
def get_param(hy, param):
    if param[0] == "gamma":
        return float(hy.gamma[param[1]])
    if param[0] == "alpha":
        return float(hy.alpha[param[1], param[2]])
    if param[0] == "beta":
        return float(hy.beta[param[1]])
    raise ValueError(param)


def set_param(hy, param, x):
    if param[0] == "gamma":
        hy.gamma[param[1]] = x
    elif param[0] == "alpha":
        hy.alpha[param[1], param[2]] = x
    elif param[0] == "beta":
        hy.beta[param[1]] = x
    else:
        raise ValueError(param)


def plant_counts(model, M, amount):
    """Add `amount` to every non-zero n_wk cell of an oracle or a sampler (after build_counts); n_k = the column sums."""
    for m in range(M):
        nwk, _ = model.get_counts(m)
        big = nwk.astype(np.int64) + np.int64(amount) * (nwk > 0)
        nk = big.sum(axis=0)
        assert nk.max() <= (1 << 30), f"planted n_k of view {m} reaches {int(nk.max())}"
        model.set_counts(m, big.astype(np.int32), nk.astype(np.int32))


def longest_first(doc_off):
    """the live sweep's work-queue order: entities by decreasing token count over all views, ties in entity order"""
    tot = sum(np.diff(np.asarray(o)) for o in doc_off)
    return np.argsort(-tot, kind="stable").astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Outcome:
    z: list
    stats: dict
    dbg: list = None

    @property
    def key(self):
        return b"".join(a.tobytes() for a in self.z)

    def branch(self, m, i):
        """0 new topic, 1 count branch, 2 tree branch of token i of view m (needs dbg)"""
        new, mass, _, s0 = self.dbg[m][i]
        if s0 < new:
            return 0
        return 1 if s0 - new < mass else 2


class Evaluator:
    """One sweep of the oracle from the case's initial assignments, as a function of one hyper-parameter.
    live = None: the deferred sweep (Oracle.sweep).  live = dict(rows=, cell16=): Oracle.sweep_live_seq, one segment."""

    def __init__(self, case, seed, live=None, plant=0, sweep_idx=0):
        self.case, self.seed, self.live, self.plant, self.sweep_idx = case, int(seed), live, int(plant), int(sweep_idx)
        self.o = Oracle(case.K, case.V)
        for m in range(case.M):
            self.o.set_corpus(m, case.doc_off[m], case.tokens[m])
        self.order = longest_first(case.doc_off) if live is not None else np.arange(case.D, dtype=np.int64)
        self.rank = np.empty(case.D, dtype=np.int64)
        self.rank[self.order] = np.arange(case.D)
        self.n_eval = 0

    def hyper_at(self, param, x):
        hy = self.case.hy.copy()
        set_param(hy, param, x)
        return hy

    def prepare(self, model, hy, set_hyper):
        """bring an oracle or a sampler to the state before the sweep"""
        set_hyper(hy)
        for m in range(self.case.M):
            model.set_assignments(m, self.case.z0[m])
        model.build_counts()
        if self.plant:
            plant_counts(model, self.case.M, self.plant)

    def run(self, param, x, want_dbg=False):
        o = self.o
        hy = self.hyper_at(param, x)
        self.prepare(o, hy, lambda h: o.set_hyper(h.alpha, h.alpha_sum, h.beta, h.beta_sum, h.gamma, h.p_a, h.p_b, h.inactive))
        self.n_eval += 1
        if self.live is None:
            r = o.sweep(self.sweep_idx, self.seed, want_dbg=want_dbg)
        else:
            assert not want_dbg
            r = o.sweep_live_seq(self.sweep_idx, self.seed, self.order, nseg=1, rows=self.live["rows"], cell16=self.live["cell16"])
        return Outcome([o.get_assignments(m) for m in range(self.case.M)], r["stats"], r.get("dbg"))


def bisect(ev, param, lo, hi, key=None):
    """(lo, hi) adjacent doubles whose outcomes differ under `key` (default: every assignment), or None when the
    ends of the interval agree."""
    key = key or (lambda out: out.key)
    want_dbg = ev.live is None
    kl, kh = key(ev.run(param, lo, want_dbg)), key(ev.run(param, hi, want_dbg))
    if kl == kh:
        return None
    while np.nextafter(lo, hi) != hi:
        mid = lo + (hi - lo) * 0.5
        if not (lo < mid < hi):
            mid = float(np.nextafter(lo, hi))
        if key(ev.run(param, mid, want_dbg)) == kl:
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


# ---------------------------------------------------------------------------------------------------------------------
# where a flip is
def token_of(case, m, i):
    d = int(np.searchsorted(case.doc_off[m], i, side="right") - 1)
    return d, m, int(i - case.doc_off[m][d])


def differing_tokens(ev, za, zb):
    """(entity, view, position) of every token whose topic differs, in the order the sweep visits them"""
    out = []
    for m in range(ev.case.M):
        for i in np.flatnonzero(za[m] != zb[m]):
            out.append(token_of(ev.case, m, int(i)))
    out.sort(key=lambda t: (int(ev.rank[t[0]]), t[1], t[2]))
    return out


def replay(case, z_after, d):
    """The entity's bookkeeping while the sweep walks it (WRK:327-391, 434-468, 557-560): before each token is sampled
    -- its old topic already taken out -- yields (view, position, token index, counts [M][K], alive [K]).  z_after =
    the assignments after the sweep.  A topic leaves the list when its count reaches zero in every view and never
    comes back (WRK:563-584 never adds).  The list is in topic order, so a topic's slot in the register kernels is its
    rank among the topics alive at the start and its place in the dense list its rank among those alive now."""
    K, M = case.K, case.M
    cnt = np.zeros((M, K), dtype=np.int64)
    span = [(int(case.doc_off[m][d]), int(case.doc_off[m][d + 1])) for m in range(M)]
    for m in range(M):
        zz = case.z0[m][span[m][0]:span[m][1]]
        np.add.at(cnt[m], zz[zz >= 0], 1)
    tot = cnt.sum(axis=0)
    alive = tot > 0
    for m in range(M):
        b, e = span[m]
        for p in range(e - b):
            if case.tokens[m][b + p] >= case.V[m]:
                continue
            old = int(case.z0[m][b + p])
            if old >= 0:
                cnt[m, old] -= 1
                tot[old] -= 1
                if tot[old] == 0:
                    alive[old] = False
            yield m, p, b + p, cnt, alive
            new = int(z_after[m][b + p])
            cnt[m, new] += 1
            tot[new] += 1


def topic_list_at(case, z_after, d, mt, pos):
    """(the entity's topics at its start, those still alive when token (d, mt, pos) is sampled), both in list order"""
    dense0 = None
    for m, p, _, cnt, alive in replay(case, z_after, d):
        if dense0 is None:
            start = alive.copy()
            old = int(case.z0[m][case.doc_off[m][d] + p])
            if old >= 0:
                start[old] = True                   # (the first token's own topic was alive before it was taken out)
            dense0 = [int(k) for k in np.flatnonzero(start)]
        if (m, p) == (mt, pos):
            return dense0, [int(k) for k in np.flatnonzero(alive)]
    raise ValueError("no such token")


@dataclass
class Flip:
    param: tuple
    lo: float
    hi: float
    kind: str                   # deferred: A, B, C, D.  live: "count", "tree"
    token: tuple                # (entity, view, position) of the first token whose topic differs
    topics: tuple               # its topic at lo and at hi
    slots: tuple = None         # kind C / count: slots (positions in the entity's initial list) of the two topics, ascending
    live_pos: int = None        # ... position of the lower one in the list of topics still alive
    n_live: int = None
    n_differ: int = 0
    seed: int = 0

    @property
    def first_slot(self):
        return self.live_pos == 0

    @property
    def last_slot(self):
        return self.live_pos is not None and self.live_pos + 2 == self.n_live

    def lane_change(self, R):
        """register kernels, slot = lane * R + r: the boundary lies between two lanes"""
        return self.slots is not None and self.slots[0] // R != self.slots[1] // R

    @property
    def block_change(self):
        """generic kernel, the list scanned in blocks of 64 slots (a dropped topic keeps its slot): the boundary lies between two blocks"""
        return self.lane_change(WAVE)


def classify(ev, param, lo, hi):
    """The flip (lo, hi) by its first differing token; None when the ends agree or the oracle abandoned an entity."""
    want_dbg = ev.live is None
    a, b = ev.run(param, lo, want_dbg), ev.run(param, hi, want_dbg)
    if a.stats["aborted_docs"] or b.stats["aborted_docs"]:
        return None
    diff = differing_tokens(ev, a.z, b.z)
    if not diff:
        return None
    d, m, pos = diff[0]
    i = int(ev.case.doc_off[m][d]) + pos
    ta, tb = int(a.z[m][i]), int(b.z[m][i])
    dense0, alive = topic_list_at(ev.case, a.z, d, m, pos)
    f = Flip(param, lo, hi, "?", (d, m, pos), (ta, tb), n_differ=len(diff), seed=ev.seed)
    both_listed = ta in alive and tb in alive
    if both_listed:
        pa, pb = sorted((alive.index(ta), alive.index(tb)))
        adjacent = pb == pa + 1
    if want_dbg:
        br = {a.branch(m, i), b.branch(m, i)}
        f.kind = "A" if 0 in br else "B" if br == {1, 2} else "C" if br == {1} else "D"
        if f.kind == "C" and both_listed and adjacent:
            f.slots = tuple(sorted((dense0.index(ta), dense0.index(tb))))
            f.live_pos, f.n_live = pa, len(alive)
    else:
        # No debug rows on the live path, so this is a HEURISTIC, not a reading: a topic outside the entity's list can only come
        # from the tree branch (the live cases have no inactive topic).  Two neighbours of the list are taken for a boundary of
        # the count branch unless the ends' branch counters show a token moving between branches or the two topics are
        # consecutive numbers -- a near-tie of the tree branch lies between two neighbouring leaves -- ; such flips stay "?".
        moved = any(a.stats[k] != b.stats[k] for k in ("topic_doc_mass_cnt", "word_ftree_mass_cnt"))
        if not both_listed:
            f.kind = "tree"
        elif adjacent and not moved and abs(ta - tb) > 1:
            f.kind = "count"
            f.slots = tuple(sorted((dense0.index(ta), dense0.index(tb))))
            f.live_pos, f.n_live = pa, len(alive)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# searches
@dataclass(frozen=True)
class Search:
    """any: bisect [lo, hi] on every assignment; the flip is wherever the first change is, so its kind follows the number
    of comparisons of each kind: with a list of S topics, S - 1 slot boundaries to one of kind A and one of kind B.
    A, B, first, last, lane, block: aim at ONE comparison of the first token of every entity.  Nothing precedes that token in its
    entity, so its decision is a monotone step of the parameter wherever the parameter moves one side of the comparison:
    with rank = -1 for the new-topic branch, the place in the list for the count branch and the list's length for the tree
    branch, the comparison with cum[b] is `rank <= b`; A is b = -1, first b = 0, last b = n - 2, B b = n - 1.
    The interval may be wide: alpha[m][K] moves newMass through every u, beta[m] the tree's share of the total."""
    param: tuple
    lo: float
    hi: float
    target: str = "any"
    seed: int = 5


def _rank_key(case, d, target):
    i = int(case.doc_off[0][d])
    dense0, alive = topic_list_at(case, case.z0, d, 0, 0)     # (nothing was sampled before the first token)
    n = len(alive)
    if n < 3:
        return None
    if target in ("lane", "block"):       # between slots 15 and 16: two lanes of every register variant; 63 and 64: two blocks of the generic scan
        edge = 16 if target == "lane" else WAVE
        slot = [dense0.index(k) for k in alive]
        b = max((j for j in range(n - 1) if slot[j] < edge <= slot[j + 1]), default=None)
        if b is None:
            return None
    else:
        b = {"A": -1, "first": 0, "last": n - 2, "B": n - 1}[target]
    place = {k: j for j, k in enumerate(alive)}

    def key(out):
        br = out.branch(0, i)
        rank = -1 if br == 0 else n if br == 2 else place.get(int(out.z[0][i]), n)
        return rank <= b
    return key


def find_flips(ev, searches, cap=None):
    """Run the searches in order; the flips found, without duplicates.  A search may find none.  cap = {kind: n}: a kind
    that has n flips gets no more, and searches that aim at it are not run (the list stays fixed, the work bounded)."""
    flips, seen, have = [], set(), {}
    case = ev.case
    cap = cap or {}
    full = lambda kind: have.get(kind, 0) >= cap.get(kind, 1 << 30)
    for s in searches:
        ev.seed = int(s.seed)
        if s.target == "any":
            pairs = [] if cap and all(full(k) for k in cap) else [bisect(ev, s.param, float(s.lo), float(s.hi))]
        else:
            assert ev.live is None, "aiming reads debug rows, which the live oracle does not write"
            pairs = []
            for d in range(case.D):
                if case.doc_off[0][d + 1] == case.doc_off[0][d] or case.tokens[0][case.doc_off[0][d]] >= case.V[0]:
                    continue
                if s.target in ("A", "B") and full(s.target):
                    continue
                if s.target not in ("A", "B") and sum(pr is not None for pr in pairs) >= 3:
                    break                                    # (three slot boundaries of a kind from one search are plenty)
                key = _rank_key(case, d, s.target)
                if key is not None:
                    pairs.append(bisect(ev, s.param, float(s.lo), float(s.hi), key=key))
        for pr in pairs:
            if pr is None or (s.seed, s.param, pr[0]) in seen:
                continue
            f = classify(ev, s.param, *pr)
            if f is not None and not (s.target in ("any", "A", "B") and full(f.kind)):
                seen.add((s.seed, s.param, pr[0]))
                have[f.kind] = have.get(f.kind, 0) + 1
                flips.append(f)
    return flips


# ---------------------------------------------------------------------------------------------------------------------
# ladders
J_MAX = 40          # 2^40 ulp: past the widest tolerance a sampler uses, a screen of 2^-17 relative (53 - 17 = 36)


@dataclass
class Rung:
    x: float
    j: int              # -1: the flip's own end
    side: str           # "lo" / "hi"
    stats: dict = field(default=None, repr=False)


def ladder_values(flip, js=None):
    ulp = flip.hi - flip.lo
    out = [Rung(flip.lo, -1, "lo"), Rung(flip.hi, -1, "hi")]
    for j in (range(J_MAX + 1) if js is None else js):
        out.append(Rung(flip.lo - 2.0 ** j * ulp, j, "lo"))
        out.append(Rung(flip.hi + 2.0 ** j * ulp, j, "hi"))
    return out


def ladder(ev, flip, js=None, dropped=None):
    """The rungs of a flip, each after the oracle's sweep at its value (ev.o holds the state after it; rung.stats the
    oracle's statistics).  A rung at which the oracle abandons an entity is left out and counted in dropped[0]."""
    ev.seed = int(flip.seed)
    for r in ladder_values(flip, js):
        out = ev.run(flip.param, r.x)
        if out.stats["aborted_docs"]:
            if dropped is not None:
                dropped[0] += 1
            continue
        r.stats = out.stats
        yield r


# ---------------------------------------------------------------------------------------------------------------------
# the fixed cases and searches of the tests
def _lens(rng, D, lam, floor=1):
    return np.maximum(rng.poisson(lam, D), floor)


def case_small():
    """two views, three inactive topics, lists of at most 64 topics: every register variant and the generic kernel"""
    rng = np.random.RandomState(11)
    return make_case("small", 40, [300, 40], [_lens(rng, 10, 100), _lens(rng, 10, 8)], 11, 36, n_inactive=3, alpha_new=2.0)


def case_mid2():
    """two views, lists of 65 to 128 topics with K and the entities beyond 64: the 2-round variant, and no narrower one"""
    rng = np.random.RandomState(16)
    return make_case("mid2", 200, [400, 40], [_lens(rng, 6, 210, 180), _lens(rng, 6, 10)], 16, 125, n_inactive=3, alpha_new=12.0)


def case_mid4():
    """five views, lists of 129 to 256 topics: the 4-round variant, and no narrower one"""
    rng = np.random.RandomState(17)
    return make_case("mid4", 400, [400, 30, 30, 30, 30], [_lens(rng, 4, 470, 420)] + [_lens(rng, 4, 8) for _ in range(4)], 17, 270,
                     n_inactive=3, alpha_new=30.0)


def case_wide8():
    """K = 1000, entities of more than 1000 tokens whose lists fit the 8-round variant (at most 512 slots)"""
    rng = np.random.RandomState(12)
    return make_case("wide8", 1000, [300, 20, 20], [1001 + rng.randint(0, 8, 2), _lens(rng, 2, 12), _lens(rng, 2, 12)], 12, 440,
                     n_inactive=3, alpha_new=90.0)


def case_wide16():
    """the corner of the screen's error budget: eight views and lists for the 16-round variant (at most 1024 slots)"""
    rng = np.random.RandomState(13)
    return make_case("wide16", 1000, [300] + [20] * 7, [1001 + rng.randint(0, 8, 2)] + [_lens(rng, 2, 9) for _ in range(7)], 13, 900,
                     n_inactive=3, alpha_new=30.0)


def case_live():
    """no inactive topic (a topic outside the entity's list then comes from the tree branch alone)"""
    rng = np.random.RandomState(14)
    return make_case("live", 200, [400, 50], [_lens(rng, 30, 60), _lens(rng, 30, 6)], 14, 24)


def searches_deferred(case):
    """The fixed searches of a deferred case: aimed ones for the comparisons a long list makes rare, plain ones for the rest.
    (An aimed search visits the first token of every entity; between a quarter and two thirds of them cross the comparison
    within the interval.)"""
    K, M, D = case.K, case.M, case.D
    aK = float(case.hy.alpha[0, K])
    out = []
    for r in range(-(-18 // D)):
        m = 0 if r % 2 == 0 else r % M
        out.append(Search(("alpha", m, K), aK / 64, aK * 4096, "A", 5 + r))
        if r < 1:
            out.append(Search(("alpha", m, K), aK / 64, aK * 4096, "first", 5 + r))
            out.append(Search(("alpha", m, K), aK / 64, aK * 4096, "lane", 5 + r))
            out.append(Search(("alpha", m, K), aK / 64, aK * 4096, "block", 5 + r))
    for r in range(-(-45 // D)):
        out.append(Search(("gamma", 0), 1.0 / 16, 16.0, "B", 20 + r))
        if r < 2:
            out.append(Search(("gamma", 0), 1.0 / 16, 16.0, "last", 20 + r))
    params = [("gamma", 0), ("gamma", M - 1), ("alpha", 0, K), ("alpha", 0, 7), ("beta", 0)]
    for r in range(12):
        p = params[r % len(params)]
        x0 = get_param(case.hy, p) * (1.0 + 0.03125 * r)
        out.append(Search(p, x0, x0 * (1.0 + 2.0 ** -5), "any", 60 + r))
    return out


DEFERRED_CAP = {"A": 8, "B": 8, "C": 12, "D": 2}


def searches_live(case):
    """The live oracle writes no debug rows: plain searches only, their kinds as they fall."""
    M = case.M
    params = [("gamma", 0), ("alpha", 0, 7), ("beta", 0), ("gamma", M - 1), ("alpha", 0, 31), ("beta", M - 1)]
    out = []
    for r in range(60):
        p = params[r % len(params)]
        x0 = get_param(case.hy, p) * (1.0 + 0.03125 * (r // len(params)))
        out.append(Search(p, x0, x0 * (1.0 + 2.0 ** -5), "any", 80 + r))
    return out


LIVE_CAP = {"count": 8, "tree": 8, "?": 2}
LIVE_FORMS = [dict(rows=1, cell16=0), dict(rows=1, cell16=1), dict(rows=0, cell16=0), dict(rows=0, cell16=1)]


def case_single():
    """one view, a large vocabulary"""
    rng = np.random.RandomState(15)
    return make_case("single", 100, [2000], [_lens(rng, 8, 130)], 15, 50, n_inactive=2, alpha_new=6.0)


# rungs of the thinned ladder: every j through the certified tolerance (j about 6..12), every second one from there to 2^40
THIN_JS = list(range(0, 13)) + list(range(14, J_MAX + 1, 2))
# ... of the cases with lists of hundreds of topics, where a sweep costs milliseconds: every second j, every fourth between
# the certified tolerance and the screen's (j about 36), where nothing changes hands
WIDE_JS = list(range(0, 13, 2)) + [16, 20, 24, 28] + list(range(32, J_MAX + 1, 2))

# Deferred cases and the register variant forced on each.  The planner gives a forced primary no more rounds than the longest
# entity could need (64 * RMAX / 2 < min(K, its tokens)), and a variant serves an entity only if its list fits (S_used <= 64 * RMAX);
# every list here is also too long for the next narrower variant.  tests/helpers.py::served_class asks the planner itself.
# The default dispatch, the generic kernel and the exact chain run on all of them.
DEFERRED_PLAN = {"single": (case_single, [1]), "small": (case_small, [1]), "mid2": (case_mid2, [2]), "mid4": (case_mid4, [4]),
                 "wide8": (case_wide8, [8]), "wide16": (case_wide16, [16])}


def deferred_flips(name, plant=0, case=None, cap=None):
    case = case or DEFERRED_PLAN[name][0]()
    ev = Evaluator(case, 5, plant=plant)
    return ev, find_flips(ev, searches_deferred(case), cap or DEFERRED_CAP)


def live_flips(form):
    case = case_live()
    ev = Evaluator(case, 5, live=form)
    return ev, find_flips(ev, searches_live(case), LIVE_CAP)


def check_deferred_quotas(flips, forced, wide=False):
    """the conditions a deferred case must meet before its ladders mean anything"""
    n = {k: sum(f.kind == k for f in flips) for k in "ABCD"}
    assert min(n["A"], n["B"], n["C"]) >= 8, n
    cs = [f for f in flips if f.kind == "C"]
    assert any(f.first_slot for f in cs) and any(f.last_slot for f in cs), "no slot boundary at the first / last live slot"
    for R in forced:
        assert any(f.lane_change(R) for f in cs), f"no slot boundary between two lanes of the {R}-round variant"
    if wide:
        assert any(f.block_change for f in cs), "no slot boundary between two blocks of the generic kernel's scan"


def check_live_quotas(flips):
    """(the kinds of live flips are inferred, see classify: "tree" is certain, "count" excludes what can be told apart)"""
    n = {k: sum(f.kind == k for f in flips) for k in ("count", "tree")}
    assert n["count"] >= 8 and n["tree"] >= 8, n
