"""MVHDP_SWEEP_SHARD_BIRTHS: the births of a truncated HDP on document shards.  The reference's updater takes a topic out of
inActiveTopicIndex with the first delta that reaches it (UPD:263-270) and its samplers then draw the next inactive index (WRK:522-526).
A shard's NO_APPLY live sweep does the same chunk by chunk, activates nothing, and leaves a per-topic table of first-delta keys
(MVHDP_BUF_BIRTH_KEYS); the shards MIN-reduce the tables and every replica activates what any shard reached (mvhdp_activate_births)."""
import numpy as np
import pytest

from mvtopicmodel_amd import NativeGroup
from mvtopicmodel_amd._lib import MvhdpError
from mvtopicmodel_amd.native import (ACT_KEY_NONE, BUF_BIRTH_KEYS, BUF_DELTA, Hyper, SWEEP_FROZEN, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS,
                                     SWEEP_NO_APPLY, SWEEP_ONLY_SEGMENT, SWEEP_SHARD_BIRTHS)
from tests.helpers import assert_same_state, make_native, make_oracle, recount, shards_of, small_corpus
from tests.near_ties import longest_first

pytestmark = pytest.mark.gpu

K, V = 60, [500, 60]
FIRST_INACTIVE = 40
BIRTHS = SWEEP_NO_APPLY | SWEEP_LIVE | SWEEP_SHARD_BIRTHS


def _model():
    """The corpus of test_gpu_live.py's births test: topics 40-59 inactive, a new-topic mass that is drawn often."""
    c = small_corpus(K, V, 400, [40, 6], 45)
    inactive = np.zeros(K, dtype=np.uint8); inactive[FIRST_INACTIVE:] = 1
    hy = Hyper.defaults(K, V, inactive=inactive); hy.alpha[:, K] = 50.0
    o = make_oracle(c, hy)
    z = [o.get_assignments(m) for m in range(c.M)]
    for m in range(c.M):
        z[m][z[m] >= FIRST_INACTIVE] = 7
        o.set_assignments(m, z[m])
    o.build_counts()
    return c, hy, o, z


def _key_topic(k):
    return int(k) & 0x7FF


def _key_view(k):
    return (int(k) >> 31) & 0x7


def _check_table(keys, ina_before, M):
    """finite keys only at topics that were inactive, a prefix of the inactive list, topic field = index, view < M"""
    born = np.flatnonzero(keys != ACT_KEY_NONE)
    assert ina_before[born].all(), "a key on a topic that was active"
    assert np.array_equal(born, np.flatnonzero(ina_before)[:born.size]), "the births are not a prefix of the inactive list"
    for k in born:
        assert _key_topic(keys[k]) == k and _key_view(keys[k]) < M
    return born


def _recount_ok(c, z_by_view, samplers):
    for m in range(c.M):
        ref = np.zeros((c.V[m], K), dtype=np.int64)
        np.add.at(ref, (c.tokens[m], z_by_view[m]), 1)
        for s in samplers:
            nwk, nk = s.get_counts(m)
            assert nwk.min() >= 0 and np.array_equal(nwk, ref) and np.array_equal(nk, ref.sum(axis=0)), f"counts are not the recount of z in view {m}"


def _shards(c, hy, z, n):
    """n NativeSamplers over contiguous entity ranges balanced by token count, each holding the GLOBAL counts (a full replica)"""
    out = []
    for lo, sub, zs in shards_of(c, z, n):
        s = make_native(sub, hy, zs, doc_id_base=lo)
        for m in range(c.M):
            nwk = recount(c.tokens[m], z[m], c.V[m], K)
            s.set_counts(m, nwk, nwk.sum(axis=0))
        out.append(s)
    return out


def test_one_handle_shard_births_then_activation_equal_the_plain_live_sweep_and_the_oracle():
    """NO_APPLY | LIVE | SHARD_BIRTHS, apply_delta(-1, -1), activate_births(get_birth_keys()) is the live sweep of one handle: with one
    resident wave both are the sequential algorithm of the oracle (births chunk by chunk included), integer for integer."""
    c, hy, o, z = _model()
    a = make_native(c, hy, z)
    b = make_native(c, hy, z)
    for s in (a, b):
        s.set_tuning(live16=0, single_wave=1, live_rows=1, force_primary=1)
    order = longest_first(c.doc_off)
    born = []
    for it in range(3):
        ina_before = b.get_alpha()[1].copy()
        ro = o.sweep_live_seq(it, 5, order, nseg=1, rows=1, cell16=0)["stats"]
        sa = a.sweep(it, 5, flags=SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(1))
        sb = b.sweep(it, 5, flags=BIRTHS | SWEEP_LIVE_SEGMENTS(1))
        assert sb.activations == 0 and np.array_equal(b.get_alpha()[1], ina_before)          # nothing activated by the sweep itself
        keys = b.get_birth_keys()
        got = _check_table(keys, ina_before.astype(bool), c.M)
        b.apply_delta(-1, -1)
        b.activate_births(keys)
        born.append(got.size)
        assert got.size == sa.activations
        for st in (sa, sb):
            assert (st.tokens, st.changed) == (ro["tokens"], ro["changed"])
            assert (st.new_mass_cnt, st.topic_doc_mass_cnt, st.word_ftree_mass_cnt) == (ro["new_mass_cnt"], ro["topic_doc_mass_cnt"], ro["word_ftree_mass_cnt"])
        for s in (a, b):
            assert_same_state(o, s, c.M)
            al, ina = s.get_alpha()
            assert np.array_equal(al, o.get_alpha()) and np.array_equal(ina, o.get_inactive())
    assert born[0] > 1 and sum(born) == K - FIRST_INACTIVE, born
    a.close(); b.close()


def test_birth_table_contract_and_activation_errors():
    c, hy, o, z = _model()
    s = make_native(c, hy, z)
    ina0 = s.get_alpha()[1].astype(bool)
    # without the flag: the stored activation key alone, at its own topic
    s.sweep(0, 5, flags=SWEEP_NO_APPLY | SWEEP_LIVE)
    keys = s.get_birth_keys()
    assert np.count_nonzero(keys != ACT_KEY_NONE) <= 1
    _check_table(keys, ina0, c.M)
    s.apply_delta(-1, -1)
    assert np.array_equal(s.get_alpha()[1].astype(bool), ina0)
    # with it: a prefix of the inactive list, read through the device buffer as well
    st = s.sweep(1, 5, flags=BIRTHS)
    assert st.activations == 0
    keys = s.get_birth_keys()
    born = _check_table(keys, ina0, c.M)
    assert born.size > 1
    ptr, nbytes = s.device_buffer(BUF_BIRTH_KEYS)
    assert ptr and nbytes == 8 * K
    s.apply_delta(-1, -1)
    alpha0, inaA = s.get_alpha()
    bad = []
    k0 = int(born[0])
    t = keys.copy(); t[k0] = (int(keys[k0]) & ~0x7FF) | ((k0 + 1) & 0x7FF); bad.append(t)        # topic field is not its index
    t = keys.copy(); t[k0] = int(keys[k0]) | (7 << 31); bad.append(t)                             # view beyond M
    t = keys.copy(); t[3] = (3 << 34) | 3; bad.append(t)                                          # a key on an active topic
    t = np.full(K, ACT_KEY_NONE, dtype=np.int64); t[FIRST_INACTIVE + 1] = (1 << 34) | (FIRST_INACTIVE + 1); bad.append(t)   # not a prefix
    for t in bad:
        with pytest.raises(MvhdpError):
            s.activate_births(t)
        al, ina = s.get_alpha()
        assert np.array_equal(al, alpha0) and np.array_equal(ina, inaA), "a refused table changed the model"
    s.activate_births(None)                                   # the table as it stands on the device
    al, ina = s.get_alpha()
    newly = np.flatnonzero(inaA.astype(bool) & ~ina.astype(bool))
    assert np.array_equal(newly, born)
    assert all((al[:, t] == 50.0).sum() == 1 for t in newly)
    assert not s.trees_current()
    # the flag is refused without LIVE, with FROZEN, with ONLY_SEGMENT
    for f in (SWEEP_NO_APPLY | SWEEP_SHARD_BIRTHS, SWEEP_LIVE | SWEEP_FROZEN | SWEEP_SHARD_BIRTHS,
              BIRTHS | SWEEP_LIVE_SEGMENTS(2) | SWEEP_ONLY_SEGMENT(0)):
        with pytest.raises(MvhdpError) as e:
            s.sweep(2, 5, flags=f)
        assert e.value.code == -1
    # without NO_APPLY the flag changes nothing: the plain live sweep gives birth itself
    st = s.sweep(2, 5, flags=SWEEP_LIVE | SWEEP_SHARD_BIRTHS)
    _recount_ok(c, [s.get_assignments(m) for m in range(c.M)], [s])
    s.close()


@pytest.mark.parametrize("members,chunks,nseg", [(2, 1, 1), (2, 4, 2), (4, 4, 1), (4, 1, 2)])
def test_group_gives_birth_to_many_topics_per_exchange(members, chunks, nseg):
    c, hy, o, z = _model()
    shards = _shards(c, hy, z, members)
    with NativeGroup(shards) as g:
        g.set_exchange_chunks(chunks)
        firsts = []
        for it in range(3):
            ina_before = shards[0].get_alpha()[1].astype(bool)
            sts = g.sweep(it, 5, flags=SWEEP_LIVE | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(nseg))
            firsts.append(sts[0].activations)
            for st in sts[1:]:
                assert (st.activations, st.activated_topic, st.activated_modality, st.activation_key) == \
                       (sts[0].activations, sts[0].activated_topic, sts[0].activated_modality, sts[0].activation_key)
            al, ina = shards[0].get_alpha()
            for s in shards[1:]:
                a2, i2 = s.get_alpha()
                assert np.array_equal(a2, al) and np.array_equal(i2, ina), "the replicas disagree on alpha / inactive"
            newly = np.flatnonzero(ina_before & ~ina.astype(bool))
            assert newly.size == sts[0].activations
            assert np.array_equal(newly, np.flatnonzero(ina_before)[:newly.size])
            assert all((al[:, t] == 50.0).sum() == 1 for t in newly)
            if newly.size:
                assert sts[0].activated_topic == newly[0] and _key_topic(sts[0].activation_key) == newly[0]
            zc = [np.concatenate([s.get_assignments(m) for s in shards]) for m in range(c.M)]
            still = np.flatnonzero(ina)
            for m in range(c.M):
                assert not np.isin(zc[m], still).any(), "an assignment refers to a topic that is still inactive"
            _recount_ok(c, zc, shards)
        assert firsts[0] > 1, firsts
        assert not shards[0].get_alpha()[1].any(), "not every topic was born within three sweeps"
    for s in shards:
        s.close()


def _by_hand(shards, it, flags):
    """The group's step composed from its members: sweeps, summed deltas and MIN-reduced birth tables through the device buffers."""
    import torch
    from mvtopicmodel_amd.dist import device_int32_tensor, device_int64_tensor
    for s in shards:
        s.sweep(it, 5, flags=flags | SWEEP_NO_APPLY)
    deltas = [device_int32_tensor(*s.device_buffer(BUF_DELTA), "cuda:0") for s in shards]
    tabs = [device_int64_tensor(*s.device_buffer(BUF_BIRTH_KEYS), "cuda:0") for s in shards]
    torch.cuda.synchronize()
    total = np.sum([d.cpu().numpy().astype(np.int64) for d in deltas], axis=0).astype(np.int32)
    keys = np.min([t.cpu().numpy() for t in tabs], axis=0)
    for d in deltas:
        d.copy_(torch.from_numpy(total))
    torch.cuda.synchronize()
    for s in shards:
        s.apply_delta(-1, -1)
        s.activate_births(keys)


@pytest.mark.parametrize("members,nseg", [(2, 1), (3, 2)])
def test_group_equals_its_members_composed_by_hand(members, nseg):
    """One resident wave on every member: each member's sweep is deterministic, so the group's step (pipelined exchange, K-wide MIN-reduce,
    activation on every replica) must equal the same steps composed by hand, bit for bit -- the MIN rule and the view of alpha included."""
    c, hy, o, z = _model()
    grp = _shards(c, hy, z, members)
    hand = _shards(c, hy, z, members)
    for s in grp + hand:
        s.set_tuning(single_wave=1, live16=0, live_rows=1, force_primary=1)
    flags = SWEEP_LIVE | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(nseg)
    with NativeGroup(grp) as g:
        for it in range(3):
            g.sweep(it, 5, flags=flags)
            _by_hand(hand, it, flags)
            for a, b in zip(grp, hand):
                for m in range(c.M):
                    assert np.array_equal(a.get_assignments(m), b.get_assignments(m)), f"sweep {it}: z differs in view {m}"
                    ca, cb = a.get_counts(m), b.get_counts(m)
                    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]), f"sweep {it}: counts differ in view {m}"
                aa, ia = a.get_alpha(); ab, ib = b.get_alpha()
                assert np.array_equal(aa, ab) and np.array_equal(ia, ib), f"sweep {it}: alpha / inactive differ"
    for s in grp + hand:
        s.close()


def test_dist_sweep_all_reduce_with_shard_births():
    import os
    import torch
    import torch.distributed as dist
    from mvtopicmodel_amd.dist import GpuShard, sweep_all_reduce
    c, hy, o, z = _model()
    s = make_native(c, hy, z)
    shard = GpuShard(s, "cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29613")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        total = 0
        for it in range(3):
            ina_before = s.get_alpha()[1].astype(bool)
            st = sweep_all_reduce(shard, it, 5, flags=SWEEP_LIVE | SWEEP_SHARD_BIRTHS, force_exchange=True, pipeline=(it != 1))
            al, ina = s.get_alpha()
            newly = np.flatnonzero(ina_before & ~ina.astype(bool))
            assert newly.size == st.activations
            assert np.array_equal(newly, np.flatnonzero(ina_before)[:newly.size])
            if it == 0:
                assert newly.size > 1
            total += newly.size
            _recount_ok(c, [s.get_assignments(m) for m in range(c.M)], [s])
        assert total == K - FIRST_INACTIVE
    finally:
        dist.destroy_process_group()
    shard.close()
    s.close()
