"""What a handle records about its device buffers (mvtopicmodel_amd/csrc/mvhdp_state.h), without a GPU: the header, compiled here with the
host compiler, against the table transcribed from the assignments it replaced (tests/golden/handle_state_transitions.txt) -- every
transition from every combination of the fields --, and the closure of the initial state under the transitions taken in any order, with
the three invariants the header discusses: each holds there, or breaks first by exactly the sequence the header names."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "handle_state_transitions.txt")
FIELDS = ["have_counts", "counts_stale", "have_trees", "full_trees", "trees_inference", "last_need_full", "delta_clean", "delta_pending",
          "delta16_used", "deltas_dirty", "rows_applied", "nslots_valid", "unassigned"]
F = {name: i for i, name in enumerate(FIELDS)}
ROWS, MASK = F["rows_applied"], F["unassigned"]
NROWS, VIEWS = 2, 2                                             # rows_applied: closed -1, partial 0, complete NROWS; unassigned: a bit per view

SHIM = r"""
#include "mvhdp_state.h"
struct ModelStateProbe {
    static void load(ModelState& s, const long long* f)
    {
        s.have_counts_ = f[0]; s.counts_stale_ = f[1]; s.have_trees_ = f[2]; s.full_trees_ = f[3]; s.trees_inference_ = f[4]; s.last_need_full_ = f[5];
        s.delta_clean_ = f[6]; s.delta_pending_ = f[7]; s.delta16_used_ = f[8]; s.deltas_dirty_ = f[9]; s.rows_applied_ = f[10]; s.nslots_valid_ = f[11];
        s.unassigned_ = (uint32_t)f[12];
    }
    static void store(const ModelState& s, long long* f)
    {
        f[0] = s.have_counts_; f[1] = s.counts_stale_; f[2] = s.have_trees_; f[3] = s.full_trees_; f[4] = s.trees_inference_; f[5] = s.last_need_full_;
        f[6] = s.delta_clean_; f[7] = s.delta_pending_; f[8] = s.delta16_used_; f[9] = s.deltas_dirty_; f[10] = s.rows_applied_; f[11] = s.nslots_valid_;
        f[12] = s.unassigned_;
    }
};
#define TRANSITIONS(X) \
    X(corpus_replaced, s.corpus_replaced((int)a, b != 0)) X(assignments_replaced, s.assignments_replaced((int)a, b != 0)) \
    X(every_token_assigned, s.every_token_assigned()) X(counts_rebuilt, s.counts_rebuilt()) X(counts_went_stale, s.counts_went_stale()) \
    X(trees_built, s.trees_built(a != 0, b != 0)) X(full_trees_written, s.full_trees_written()) X(trees_outdated, s.trees_outdated()) \
    X(trees_overwritten, s.trees_overwritten()) X(sweep_planned, s.sweep_planned(a != 0)) X(delta_zeroed, s.delta_zeroed()) \
    X(delta_written, s.delta_written(a != 0)) X(delta_left_pending, s.delta_left_pending()) X(delta_applied, s.delta_applied()) \
    X(delta_discarded, s.delta_discarded(a != 0)) X(delta16_rebiased, s.delta16_rebiased()) X(overlap_enqueued, s.overlap_enqueued()) \
    X(overlap_finished, s.overlap_finished()) X(bracket_begun, s.bracket_begun()) X(bracket_rows, s.bracket_rows(a)) \
    X(bracket_closed, r = s.bracket_closed(a)) X(bracket_abandoned, s.bracket_abandoned()) X(nslots_counted, s.nslots_counted(a != 0)) \
    X(nslots_invalidated, s.nslots_invalidated())
#define NAME(n, call) #n,
#define INDEX(n, call) T_##n,
#define CASE(n, call) case T_##n: call; break;
static const char* const names[] = { TRANSITIONS(NAME) };
enum { TRANSITIONS(INDEX) };
extern "C" {
int state_transitions(void) { return (int)(sizeof names / sizeof names[0]); }
const char* state_transition_name(int t) { return names[t]; }
void state_initial(long long* f) { ModelState s; ModelStateProbe::store(s, f); }
// transition t with the arguments a, b on each of the n states at f; ret: what the transition returned (-1: nothing)
void state_apply(int t, long long a, long long b, int n, long long* f, int* ret)
{
    for (int i = 0; i < n; i++, f += 13) {
        ModelState s; ModelStateProbe::load(s, f);
        int r = -1;
        switch (t) { TRANSITIONS(CASE) }
        ModelStateProbe::store(s, f); ret[i] = r;
    }
}
// the accessors, in the order of the fields (bracket_open for rows_applied, any_unassigned for the views)
void state_read(int n, const long long* f, long long* out)
{
    for (int i = 0; i < n; i++, f += 13, out += 13) {
        ModelState s; ModelStateProbe::load(s, f);
        const bool v[13] = {s.have_counts(), s.counts_stale(), s.trees_current(), s.full_trees(), s.trees_inference(), s.last_need_full(), s.delta_clean(),
                            s.delta_pending(), s.delta16_used(), s.deltas_dirty(), s.bracket_open(), s.nslots_valid(), s.any_unassigned()};
        for (int k = 0; k < 13; k++) out[k] = v[k];
    }
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the state header cannot be checked")
    d = tmp_path_factory.mktemp("state")
    src, lib = d / "state_shim.cpp", d / "libstate_shim.so"
    src.write_text(SHIM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "mvtopicmodel_amd", "csrc"), "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.state_transition_name.restype = C.c_char_p
    return L


def names(shim):
    return [shim.state_transition_name(t).decode() for t in range(shim.state_transitions())]


def apply(shim, t, a, b, states):
    """the states (rows of 13 fields) after transition t(a, b), and what it returned for each"""
    out = np.ascontiguousarray(states, dtype=np.int64).copy()
    ret = np.empty(len(out), dtype=np.int32)
    shim.state_apply(t, C.c_longlong(a), C.c_longlong(b), len(out), out.ctypes.data_as(C.c_void_p), ret.ctypes.data_as(C.c_void_p))
    return out, ret


def every_state():
    doms = [(-1, 0, NROWS) if i == ROWS else tuple(range(1 << VIEWS)) if i == MASK else (0, 1) for i in range(len(FIELDS))]
    return np.array(list(itertools.product(*doms)), dtype=np.int64)


def row_class(states):
    r = states[:, ROWS]
    return np.where(r < 0, 0, np.where(r == NROWS, 2, 1))       # closed, partial, complete


# an argument of the table -> the values it is tried with
ARG_VALUES = {"m": tuple(range(VIEWS)), "all": (-1,), "n": (0, 1, NROWS), "nrows": (NROWS,)}


def recorded():
    """[(transition, argument names, starting class, effects, returned)] as the table has them"""
    lines = []
    for line in open(TABLE):
        line = line.split("#")[0].strip()
        if not line:
            continue
        parts = [p.strip() for p in line.split("|")]
        assert len(parts) in (3, 4), line
        head = parts[0].split()
        lines.append((head[0], head[1:], parts[1].split(), parts[2].split(), int(parts[3]) if len(parts) == 4 else -1))
    return lines


def value(tok, args):
    return args[tok] if tok.startswith("$") else int(tok)


def selects(cond, args, states):
    """the states (and argument values) a line's starting class covers"""
    sel = np.ones(len(states), dtype=bool)
    for c in cond:
        if c == "*":
            continue
        if c in ("closed", "partial", "complete"):
            sel &= row_class(states) == ("closed", "partial", "complete").index(c)
            continue
        name, v = c.split("=")
        if name.startswith("$"):
            sel &= args[name] == int(v)
        else:
            sel &= states[:, F[name]] == int(v)
    return sel


def expected(effects, args, states):
    out = states.copy()
    for e in effects:
        if e == "rows_applied+=n":
            out[:, ROWS] += args["n"]
        elif e.startswith("unassigned["):
            which, v = e[len("unassigned["):].split("]=")
            bits = (1 << VIEWS) - 1 if which == "*" else 1 << args["m"]
            out[:, MASK] = (out[:, MASK] | bits) if value(v, args) else (out[:, MASK] & ~bits)
        else:
            name, v = e.split("=")
            out[:, F[name]] = value(v, args)
    return out


def test_every_transition_from_every_state_leaves_what_the_sites_it_replaced_wrote(shim):
    table = recorded()
    init = np.zeros((1, len(FIELDS)), dtype=np.int64)
    shim.state_initial(init.ctypes.data_as(C.c_void_p))
    first = [ln for ln in table if ln[0] == "initial"]
    anything = np.full((1, len(FIELDS)), 7, dtype=np.int64); anything[0, MASK] = (1 << VIEWS) - 1
    assert len(first) == 1 and np.array_equal(init, expected(first[0][3], {}, anything))               # (the table names every field)
    table = [ln for ln in table if ln[0] != "initial"]
    assert sorted(set(ln[0] for ln in table)) == sorted(names(shim))        # every transition of the header is recorded, and no other
    states = every_state()
    assert len(states) == 2 ** 11 * 3 * 2 ** VIEWS
    checked = 0
    for t, name in enumerate(names(shim)):
        lines = [ln for ln in table if ln[0] == name]
        for argnames in sorted(set(tuple(ln[1]) for ln in lines)):          # (a view and every view are two signatures of one transition)
            doms = [(0, 1) if a.startswith("$") else ARG_VALUES[a] for a in argnames]
            for vals in itertools.product(*doms):
                args = dict(zip(argnames, vals))
                a, b = (list(vals) + [0, 0])[:2]
                got, ret = apply(shim, t, a, b, states)
                covered = np.zeros(len(states), dtype=int)
                for _, an, cond, effects, returned in lines:
                    if tuple(an) != argnames:
                        continue
                    sel = selects(cond, args, states)
                    covered += sel
                    want = expected(effects, args, states[sel])
                    bad = np.flatnonzero((got[sel] != want).any(axis=1) | (ret[sel] != returned))
                    assert len(bad) == 0, (f"{name}{args} from {dict(zip(FIELDS, states[sel][bad[0]]))}: the header leaves {dict(zip(FIELDS, got[sel][bad[0]]))} "
                                           f"and returns {ret[sel][bad[0]]}, the sites left {dict(zip(FIELDS, want[bad[0]]))} and {returned}")
                assert (covered == 1).all(), f"{name}{args}: the table covers a starting state {covered.min()} or {covered.max()} times"
                checked += len(states)
    assert checked >= len(names(shim)) * len(states)
    # the accessors read the fields they are named after
    seen = np.empty_like(states)
    shim.state_read(len(states), states.ctypes.data_as(C.c_void_p), seen.ctypes.data_as(C.c_void_p))
    want = states.copy(); want[:, ROWS] = states[:, ROWS] >= 0; want[:, MASK] = states[:, MASK] != 0
    assert np.array_equal(seen, want)


# (a), (b), (c) of the header: the invariant, and the shortest sequence from the initial state that breaks it when the transitions are
# taken in any order (None: it holds in the whole closure).  mvhdp_state.h says which of these the library's own call order can take.
INVARIANTS = [
    ("delta_pending implies !delta_clean", lambda s: ~((s[:, F["delta_pending"]] == 1) & (s[:, F["delta_clean"]] == 1)),
     ["delta_zeroed()", "delta_left_pending()"]),
    ("an open bracket implies !have_trees", lambda s: ~((s[:, ROWS] >= 0) & (s[:, F["have_trees"]] == 1)),
     ["bracket_begun()", "trees_built(0, 0)"]),
    ("delta16_used implies !delta_clean", lambda s: ~((s[:, F["delta16_used"]] == 1) & (s[:, F["delta_clean"]] == 1)),
     ["delta_written(1)", "delta_zeroed()"]),
]


def test_the_closure_of_the_initial_state_and_the_three_invariants(shim):
    """Breadth first over (fields, rows_applied as closed / partial / complete).  The transitions are the former sites' writes and no more,
    so taken freely they reach every combination: what the header claims is which sequences break (a), (b), (c) first, and those it is
    held to -- a transition that learnt to refuse one of them changes the witness and fails here until the header says so."""
    table = recorded()
    actions = []                                                            # (label, t, a, b), in the table's order, every argument value
    for t, name in enumerate(names(shim)):
        for argnames in sorted(set(tuple(ln[1]) for ln in table if ln[0] == name)):
            for vals in itertools.product(*[(0, 1) if a.startswith("$") else ARG_VALUES[a] for a in argnames]):
                a, b = (list(vals) + [0, 0])[:2]
                actions.append((f"{name}({', '.join(str(v) for v in vals)})", t, a, b))

    def canonical(s):
        s[:, ROWS] = np.array([-1, 0, NROWS])[row_class(s)]
        return s

    def code(s):                                                            # one integer per state
        digits = s.copy(); digits[:, ROWS] = row_class(s)
        return (digits * np.array([1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 8192])).sum(axis=1)

    init = np.zeros((1, len(FIELDS)), dtype=np.int64)
    shim.state_initial(init.ctypes.data_as(C.c_void_p))
    before = np.full(1 << 15, -2, dtype=np.int64)                           # per state code: the code it was first reached from (-1: initial), by which action
    by = np.full(1 << 15, -1, dtype=np.int64)
    before[code(init)[0]] = -1
    frontier, reached = init, [init]
    while len(frontier):
        nxt = []
        for k, (label, t, a, b) in enumerate(actions):
            out = canonical(apply(shim, t, a, b, frontier)[0])
            c0, c1 = code(frontier), code(out)
            new, at = np.unique(np.where(before[c1] == -2, c1, -1), return_index=True)
            new, at = new[new >= 0], at[new >= 0]
            before[new] = c0[at]; by[new] = k
            nxt.append(out[at])
        frontier = np.concatenate(nxt)
        reached.append(frontier)
    reached = np.concatenate(reached)
    assert len(reached) == (before != -2).sum() == 2 ** 11 * 3 * 2 ** VIEWS  # every combination: the fields are independent of each other

    def path(c):
        steps = []
        while before[c] != -1:
            steps.append(actions[by[c]][0]); c = before[c]
        return steps[::-1]

    for what, holds, witness in INVARIANTS:
        bad = reached[~holds(reached)]
        if witness is None:
            assert len(bad) == 0, f"{what}: broken by {path(int(code(bad[:1])[0]))}"
            continue
        assert len(bad), f"{what} holds in the whole closure now: say so in mvhdp_state.h and here"
        shortest = min((path(int(c)) for c in code(bad)), key=lambda p: (len(p), p))
        assert len(shortest) == len(witness) and path_breaks(shim, witness, holds), f"{what}: first broken by {shortest}, the header names {witness}"


def path_breaks(shim, witness, holds):
    """does the named sequence, from the initial state, end in a state that breaks the invariant (and none before its end)"""
    index = {n: t for t, n in enumerate(names(shim))}
    s = np.zeros((1, len(FIELDS)), dtype=np.int64)
    shim.state_initial(s.ctypes.data_as(C.c_void_p))
    for k, step in enumerate(witness):
        if not holds(s)[0]:
            return False
        name, rest = step.rstrip(")").split("(")
        vals = [int(v) for v in rest.split(",") if v.strip()]
        a, b = (vals + [0, 0])[:2]
        s = apply(shim, index[name], a, b, s)[0]
    return not holds(s)[0]
