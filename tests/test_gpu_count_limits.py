"""The narrow forms of the word-topic counts at the exact limits their comments derive, under full swings (tests/swing_cases.py): rows of
32767, 32768, 65534 and 65535 tokens whose every token changes topic in one sweep, so that a 16-bit delta cell reaches -+32767 in both
halves of a word, a cell of the 16-bit mirror goes 65534 <-> 0, the row classes sit on their cuts, the packed group exchange carries
-+32767 summed from several members, and rows enter and leave the 12-bit image.  Every sweep mode, after EVERY step: the integers are
the oracle's where the mode has an oracle form, the closed form in any case (the outcome does not depend on the interleaving), the counts
are the recount of the assignments, and `changed` / `tokens` are the oracle's.  Integers only, no tolerance.  Each mode's witness -- the
launch census, mvhdp_plan_probe, exchange_packed, the row-class bytes -- is asserted."""
import numpy as np
import pytest

from mvtopicmodel_amd import NativeGroup
from mvtopicmodel_amd._lib import MvhdpError
from mvtopicmodel_amd.native import (BUF_COUNTS12, BUF_ROW_CLASS, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, SWEEP_SEGMENT_APPLY,
                                     SWEEP_SEGMENT_OVERLAP)
from tests import swing_cases as sw
from tests.helpers import After, assert_same_state, make_native, make_oracle, recount, shards_of
from tests.test_gpu_segmented import oracle_overlapped_sweep, oracle_segmented_sweep
from tests.test_gpu_slim_rows import device_bytes, unpack12

pytestmark = pytest.mark.gpu
SEED = 77
STEPS = range(len(sw.TARGETS))
SEGMENTS = 3
OVERLAPPED_SEGMENTS = 2                           # the largest deltas a segment can leave: half a row each, both pending at the sweep's end


class Case:
    def __init__(self):
        self.c, self.z0 = sw.corpus()
        self.hy = [sw.hyper_for(t) for t in sw.TARGETS]
        self.want = [sw.expected_after(it, self.c) for it in STEPS]
        self.follow_up = sw.expected_for(sw.FOLLOW_UP, self.c)


@pytest.fixture(scope="module")
def case():
    return Case()


def set_oracle_hyper(o, hy):
    o.set_hyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)


def oracle_chain(case, z0, sweep):
    """[(statistics, the state after, n_wk of every row before)] per step of the oracle's chain; sweep(o, it) -> statistics"""
    c = case.c
    o = make_oracle(c, case.hy[0])
    for m in range(c.M):
        o.set_assignments(m, z0[m])
    o.build_counts()
    out = []
    for it in STEPS:
        set_oracle_hyper(o, case.hy[it])
        before = np.concatenate([o.get_counts(m)[0] for m in range(c.M)])
        st = sweep(o, it)
        out.append((st, After(o, c.M), before))
    o.close()
    return out


@pytest.fixture(scope="module")
def deferred(case):
    return oracle_chain(case, case.z0, lambda o, it: o.sweep(it, SEED)["stats"])


@pytest.fixture(scope="module")
def segmented(case):
    return oracle_chain(case, case.z0, lambda o, it: oracle_segmented_sweep(o, case.c, it, SEED, SEGMENTS)[0])


@pytest.fixture(scope="module")
def overlapped(case):
    return oracle_chain(case, case.z0, lambda o, it: oracle_overlapped_sweep(o, case.c, it, SEED, OVERLAPPED_SEGMENTS))


@pytest.fixture(scope="module")
def guarded(case):
    """the deferred chain from the start with a tenth of type 0's tokens unassigned"""
    return oracle_chain(case, sw.guard_start(case.c, case.z0), lambda o, it: o.sweep(it, SEED)["stats"])


def native(case, z=None, **tuning):
    s = make_native(case.c, case.hy[0], case.z0 if z is None else z)
    s.set_tuning(**dict(sw.TUNING, **tuning))
    s.sweep_census(enable=True, reset=True)
    return s


def check_state(case, handles, want, after, where):
    """handles: one sampler, or the members of a group in entity order (z concatenated, every replica's counts)"""
    c = case.c
    z = [np.concatenate([s.get_assignments(m) for s in handles]) for m in range(c.M)]
    for m in range(c.M):
        bad = np.flatnonzero(z[m] != want[0][m])
        assert not len(bad), f"{where}: z of view {m} is not the closed form in {len(bad)} tokens; their types {np.bincount(c.tokens[m][bad], minlength=c.V[m]).tolist()}, " \
                             f"their topics {dict(zip(*[a.tolist() for a in np.unique(z[m][bad], return_counts=True)]))}"
        ref = recount(c.tokens[m], z[m], c.V[m], c.K)
        for i, s in enumerate(handles):
            nwk, nk = s.get_counts(m)
            bad = np.argwhere(nwk != want[1][m][0])
            assert not len(bad), f"{where}: n_wk of view {m}, member {i}: (row, cell) {bad[:6].tolist()} hold {nwk[tuple(bad[:6].T)].tolist()}"
            assert np.array_equal(nk, want[1][m][1]), f"{where}: n_k of view {m}, member {i}"
            assert np.array_equal(nwk, ref) and np.array_equal(nk, ref.sum(axis=0)), f"{where}: the counts are not the recount of z"
    if after is not None:
        assert len(handles) == 1
        try:
            assert_same_state(after, handles[0], c.M)
        except AssertionError as e:
            raise AssertionError(f"{where}: {e}") from None


def check_stats(rs, st, where):
    """rs: the statistics of one sweep, or of every member of a group"""
    rs = rs if isinstance(rs, list) else [rs]
    assert (sum(r.tokens for r in rs), sum(r.changed for r in rs)) == (st["tokens"], st["changed"]), where
    assert all(r.aborted_docs == 0 and r.oov_skipped == 0 for r in rs), where


def census_narrow(s, sampled, where, only=None):
    """every sampled token under a key with narrow != 0 (only: under keys with exactly that narrow); the census starts afresh"""
    rows = [r for r in s.sweep_census() if r.tokens or r.launches]
    s.sweep_census(reset=True)
    text = "\n".join(f"  {r.key}: {r.launches} launches, {r.tokens} tokens" for r in rows)
    assert sum(r.tokens for r in rows) == sampled > 0, f"{where}: the census counted other tokens than the sweeps' {sampled}\n{text}"
    for r in rows:
        if r.tokens:
            assert r.key[0] != 0 and (r.key[3] != 0 if only is None else r.key[3] == only), f"{where}: tokens sampled by {r.key}\n{text}"
    return {r.key for r in rows if r.tokens}


def check_rows(s, nwk_all, slim_handle, where):
    """MvModel::heavy and the 12-bit image as the last tree build left them, against the counts it saw"""
    K = nwk_all.shape[1]
    cls = device_bytes(s, BUF_ROW_CLASS).cpu().numpy()
    want = sw.row_classes(nwk_all)
    assert np.array_equal(cls & 3, want & 3), f"{where}: row classes {(cls & 3).tolist()}, totals {nwk_all.sum(axis=1).tolist()}"
    if not slim_handle:
        assert not (cls & sw.ROW_SLIM).any(), where
        with pytest.raises(MvhdpError):
            s.device_buffer(BUF_COUNTS12)
        return
    assert np.array_equal(cls & sw.ROW_SLIM, want & sw.ROW_SLIM), f"{where}: slim bits {(cls & 4).tolist()}, largest cells {nwk_all.max(axis=1).tolist()}"
    slim = (want & sw.ROW_SLIM) != 0
    img = device_bytes(s, BUF_COUNTS12).cpu().numpy().reshape(-1, 128 * ((K + 84) // 85))
    assert np.array_equal(unpack12(img[slim], K), nwk_all[slim]), f"{where}: the 12-bit image of the slim rows"


def follow_up(case, s, it, where):
    """a plain deferred sweep to a new target on the handle as the mode left it: it gathers from the mirror the mode kept"""
    s.set_hyper(sw.hyper_for(sw.FOLLOW_UP))
    rs = s.sweep(it, SEED)
    check_stats(rs, dict(tokens=case.c.total_tokens, changed=case.c.total_tokens), where)
    check_state(case, [s], case.follow_up, None, where)
    census_narrow(s, rs.tokens, where)


# ---- plain deferred sweeps on the narrow kernels: the 16-bit delta cells, the row classes, the 12-bit image ----
@pytest.mark.parametrize("env", [{"MVHDP_DELTA16": "1"}, {"MVHDP_DELTA16": "0"}, {"MVHDP_SLIM": "0"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
@pytest.mark.parametrize("force", [0, 1, 2])
def test_deferred_swings_on_the_narrow_kernels(case, deferred, monkeypatch, force, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = native(case, force_primary=force)
    slim_handle = env.get("MVHDP_SLIM") != "0"
    first = sw.row_classes(deferred[0][2])
    assert np.array_equal(first[:sw.V[0]] & 3, [0, 0, 0, sw.ROW_BIG, sw.ROW_BIG, sw.ROW_HEAVY, 0, 0, 0])
    sampled, slim_seen = 0, []
    for it in STEPS:
        where = f"deferred, force_primary {force}, {env}, step {it}"
        s.set_hyper(case.hy[it])
        rs = s.sweep(it, SEED)
        st, after, before = deferred[it]
        check_stats(rs, st, where)
        check_state(case, [s], case.want[it], after, where)
        check_rows(s, before, slim_handle, where)
        slim_seen.append(sw.row_classes(before) & sw.ROW_SLIM)
        sampled += rs.tokens
    keys = census_narrow(s, sampled, f"deferred, force_primary {force}, {env}")
    assert {k[3] for k in keys} == ({2} if slim_handle else {1}), keys          # (K = 257: the 12-bit image pays, and every entity's kernel has the flavour)
    # rows left the image at the first swing: the spread type, and the type whose largest cell went from 4095 to 4096
    assert slim_seen[0][6] and slim_seen[0][8] and not slim_seen[2][6] and not slim_seen[2][8]
    # ... and the classes and the image once more after the last swing
    s.build_trees()
    check_rows(s, np.concatenate([w[0] for w in case.want[STEPS[-1]][1]]), slim_handle, "after the last swing")
    s.close()


# ---- deltas that leave the sweep: NO_APPLY + apply_delta, and the bracket row range by row range ----
@pytest.mark.parametrize("how", ["apply_delta", "bracket"])
def test_no_apply_swings_and_their_apply_pass(case, deferred, how):
    s = native(case)
    rows = sum(sw.V)
    # the bracket's ranges: cut inside view 0, at the view border, and inside view 1
    ranges = [(0, 4), (4, sw.V[0]), (sw.V[0], sw.V[0] + 1), (sw.V[0] + 1, rows)]
    sampled = 0
    for it in STEPS:
        where = f"NO_APPLY + {how}, step {it}"
        s.set_hyper(case.hy[it])
        held = [s.get_counts(m) for m in range(case.c.M)]
        rs = s.sweep(it, SEED, flags=SWEEP_NO_APPLY)
        for m in range(case.c.M):                                           # the deltas are pending: the counts are the sweep's start
            a, b = s.get_counts(m)
            assert np.array_equal(a, held[m][0]) and np.array_equal(b, held[m][1]), where
        if how == "apply_delta":
            s.apply_delta(-1, -1)
        else:
            s.apply_delta_begin()
            for r0, r1 in (ranges if it % 2 == 0 else ranges[::-1]):
                s.apply_delta_rows(r0, r1)
            s.apply_delta_end(-1, -1)
            assert s.trees_current() == 1
        st, after, _ = deferred[it]
        check_stats(rs, st, where)
        check_state(case, [s], case.want[it], after, where)
        sampled += rs.tokens
    census_narrow(s, sampled, f"NO_APPLY + {how}")
    s.close()


# ---- segments with the updater in between, and beside the samplers ----
def test_segmented_swings(case, segmented):
    s = native(case)
    sampled = 0
    for it in STEPS:
        where = f"segmented, step {it}"
        s.set_hyper(case.hy[it])
        rs = s.sweep(it, SEED, flags=SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(SEGMENTS))
        st, after, _ = segmented[it]
        check_stats(rs, st, where)
        check_state(case, [s], case.want[it], after, where)
        sampled += rs.tokens
    census_narrow(s, sampled, "segmented")
    follow_up(case, s, len(STEPS), "a deferred sweep behind the segmented swings")
    s.close()


def test_overlapped_segments_keep_the_mirror_by_packed_deltas(case, overlapped):
    """apply2_counts_kernel's packed add into the mirror with whole-row deltas in both halves of a word; a corrupt mirror shows in the
    deferred sweep that follows"""
    s = native(case)
    sampled = 0
    for it in STEPS:
        where = f"overlapped segments, step {it}"
        s.set_hyper(case.hy[it])
        rs = s.sweep(it, SEED, flags=SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP | SWEEP_LIVE_SEGMENTS(OVERLAPPED_SEGMENTS))
        st, after, _ = overlapped[it]
        check_stats(rs, st, where)
        check_state(case, [s], case.want[it], after, where)
        sampled += rs.tokens
    census_narrow(s, sampled, "overlapped segments", only=1)
    follow_up(case, s, len(STEPS), "a deferred sweep behind the overlapped segments")
    s.close()


# ---- live sweeps, fully parallel: the mirror kept current by packed 16-bit atomics ----
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("live_rows", [1, 0])
@pytest.mark.parametrize("live16", [1, 0])
def test_live_swings(case, deferred, live16, live_rows, nseg):
    """live16 = 1 with live_rows = 1 is the form in which a HEAVY word walks a stored tree that heavy_refresh_kernel rewrites beside the
    samplers.  Before the samplers refused a leaf without alpha from such a read, 48 to 93 of the 65535 tokens of type 5 ended step 0 in
    topics 254 and 126 (tree[1] of a new tree over left-child sums of an old one sends the descent right at every level: 511 - K = 254)."""
    s = native(case, live16=live16, live_rows=live_rows)
    sampled = 0
    for it in STEPS:
        where = f"live, live16 {live16}, live_rows {live_rows}, {nseg} segments, step {it}"
        s.set_hyper(case.hy[it])
        rs = s.sweep(it, SEED, flags=SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(nseg))
        check_stats(rs, deferred[it][0], where)
        check_state(case, [s], case.want[it], None, where)
        sampled += rs.tokens
    keys = census_narrow(s, sampled, f"live, live16 {live16}, live_rows {live_rows}, {nseg} segments", only=1 if live16 else 0)
    assert all((k[5] != 0) == bool(live_rows) for k in keys), keys
    follow_up(case, s, len(STEPS), f"a deferred sweep behind the live swings (live16 {live16}, live_rows {live_rows}, {nseg} segments)")
    s.close()


@pytest.mark.parametrize("live16", [1, 0])
def test_live_no_apply_swings_the_after_minus_before_pass(case, deferred, live16):
    """32-bit deltas of -+65535 made from the live counts and the sweep-start snapshot.  (live16 = 1: the live-rows form of
    test_live_swings, with its heavy word.)"""
    s = native(case, live16=live16)
    sampled = 0
    for it in STEPS:
        where = f"live + NO_APPLY, live16 {live16}, step {it}"
        s.set_hyper(case.hy[it])
        held = [s.get_counts(m) for m in range(case.c.M)]
        rs = s.sweep(it, SEED, flags=SWEEP_LIVE | SWEEP_NO_APPLY)
        for m in range(case.c.M):
            a, b = s.get_counts(m)
            assert np.array_equal(a, held[m][0]) and np.array_equal(b, held[m][1]), where
        s.apply_delta(-1, -1)
        check_stats(rs, deferred[it][0], where)
        check_state(case, [s], case.want[it], None, where)
        sampled += rs.tokens
    census_narrow(s, sampled, f"live + NO_APPLY, live16 {live16}", only=1 if live16 else 0)
    s.close()


# ---- document shards in one process: the exchange at half width ----
@pytest.mark.parametrize("exchange16", [None, "0"])
@pytest.mark.parametrize("n", [2, 3])
def test_group_swings_through_the_packed_exchange(case, deferred, monkeypatch, n, exchange16):
    """Contiguous shards cut a light row of 32767 tokens (tests/test_swing_cases.py), so the members' partial deltas add up to -+32767 in
    the leader's buffer before it is packed.  The layout is agreed on behind the idle sweep of step 1: steps 2 to 5 travel packed."""
    c = case.c
    if exchange16 is not None:
        monkeypatch.setenv("MVHDP_EXCHANGE16", exchange16)
    shards = [make_native(sub, case.hy[0], zs, doc_id_base=lo) for lo, sub, zs in shards_of(c, case.z0, n)]
    single = native(case)
    for s in shards:
        s.set_tuning(**sw.TUNING)
    with NativeGroup(shards) as g:
        g.build_counts()
        packed, nbytes = [], []
        for it in STEPS:
            where = f"group of {n}, MVHDP_EXCHANGE16 {exchange16}, step {it}"
            g.set_hyper(case.hy[it])
            single.set_hyper(case.hy[it])
            sts = g.sweep(it, SEED)
            single.sweep(it, SEED)
            info = g.info()
            packed.append(info.exchange_packed); nbytes.append(info.last_exchange_bytes)
            st, after, _ = deferred[it]
            check_stats(sts, st, where)
            check_state(case, shards, case.want[it], None, where)
            for m in range(c.M):
                assert np.array_equal(np.concatenate([s.get_assignments(m) for s in shards]), single.get_assignments(m)), where
                nwk, nk = single.get_counts(m)
                assert np.array_equal(nwk, after.get_counts(m)[0])
                for s in shards:
                    a, b = s.get_counts(m)
                    assert np.array_equal(a, nwk) and np.array_equal(b, nk), where
        # agreed on at the end of the second sweep, so the swings from step 2 on were packed (or never, when switched off)
        assert packed == ([0] * len(STEPS) if exchange16 == "0" else [0, 1] + [1] * (len(STEPS) - 2)), packed
        if exchange16 == "0":
            assert len(set(nbytes)) == 1, nbytes
        else:
            assert nbytes[0] == nbytes[1] and all(b < nbytes[0] for b in nbytes[2:]), nbytes
    for s in shards + [single]:
        s.close()


# ---- the guard: while a token may be unassigned, no 16-bit delta cells and no live mirror ----
@pytest.mark.parametrize("mode", ["deferred", "live"])
def test_unassigned_tokens_keep_the_narrow_cells_out_for_one_sweep(case, guarded, mode):
    import ctypes as C
    from mvtopicmodel_amd import _lib
    from tests.census_cases import probe_tuning
    c = case.c
    zg = sw.guard_start(c, case.z0)
    assert np.count_nonzero(zg[0] == -1) == 3277 and not (zg[1] == -1).any()
    for unassigned, want16 in ((True, 0), (False, 1)):
        po = _lib.PlanOutputC()
        assert _lib.load_library().mvhdp_plan_probe(C.byref(sw.plan_input(c, False, unassigned=unassigned)), C.byref(probe_tuning(sw.TUNING, {})), C.byref(po)) == 0
        assert po.status == 0 and po.delta16 == want16
    ref = guarded
    assert ref[0][2][0].sum() == 32767 - 3277                              # the counts are built from the rest: the first visits ADD to the row
    s = native(case, z=zg, live16=1)
    flags = SWEEP_LIVE if mode == "live" else 0
    for it in (0, 1, 2):
        where = f"guard, {mode}, step {it}"
        s.set_hyper(case.hy[it])
        rs = s.sweep(it, SEED, flags=flags)
        st, after, _ = ref[it]
        check_stats(rs, st, where)
        check_state(case, [s], case.want[it], after if mode == "deferred" else None, where)
        # a live sweep stays off the mirror while a first visit can add to a row; with everything assigned it is narrow again
        census_narrow(s, rs.tokens, where, only=(0 if it == 0 else 1) if mode == "live" else None)
    s.close()
