"""Deferred sweeps that gather slim rows from the 12-bit image of n_wk (MvModel::counts12, mvhdp_slim.h; the NARROW = 2 flavour of
sweep_fast_kernel): one view holds every class of row at once -- a word whose largest cell is exactly 4095 (slim), one at 4096 (the
16-bit mirror), one far above 65534 (the 32-bit table), a diffuse word of 40 000 tokens (big AND slim) and a diffuse word of 70 000
(heavy AND slim) --, rows change class from sweep to sweep, K sits on both sides of a multiple of 85, and every launched variant
sweeps plain and segmented.  Every integer must be the oracle's; with the table switched off (MVHDP_SLIM=0) the same library must
give the same integers again."""
import numpy as np
import pytest

from mvtopicmodel_amd.native import (BUF_COUNTS12, BUF_ROW_CLASS, Hyper, SWEEP_LIVE_SEGMENTS, SWEEP_REUSE_TREES, SWEEP_SEGMENT_APPLY)
from mvtopicmodel_amd.synth import Corpus
from mvtopicmodel_amd._lib import MvhdpError
from tests.helpers import assert_same_state, make_native, make_oracle
from tests.test_gpu_segmented import segment_lists

pytestmark = pytest.mark.gpu
STATS = ("tokens", "changed", "new_mass_cnt", "topic_doc_mass_cnt", "word_ftree_mass_cnt", "oov_skipped", "aborted_docs")
ROW_SLIM = 4


def corpus_with_every_row_class(K, seed):
    """View 0: entities of 48, 100, 220 and 700 tokens -- topic lists for the 1-, 2-, 4- and 8-round variants, the last of which has no
    12-bit flavour and runs on the mirror beside the others; types 0..4 are the five classes of the module docstring, the other 55
    types share what is left."""
    rng = np.random.RandomState(seed)
    V = [60, 5]
    lens0 = np.concatenate([np.full(3000, 48), np.full(600, 100), np.full(150, 220), np.full(10, 700)]).astype(np.int64)
    rng.shuffle(lens0)
    D, n0 = lens0.size, int(lens0.sum())
    special = {0: 70_000, 1: 4095 + 1500, 2: 4096 + 1500, 3: 40_000, 4: 70_000}
    types = np.concatenate([np.full(n, w, dtype=np.int32) for w, n in special.items()] +
                           [rng.randint(5, V[0], n0 - sum(special.values())).astype(np.int32)])
    rng.shuffle(types)
    z = rng.randint(0, K, n0).astype(np.int32)
    z[types == 0] = 3                                                   # one cell of 70 000
    for w, k, n in ((1, 5, 4095), (2, 7, 4096)):
        idx = np.flatnonzero(types == w)
        z[idx[:n]] = k
        rest = rng.randint(0, K - 1, idx.size - n).astype(np.int32)
        z[idx[n:]] = rest + (rest >= k)                                  # the others anywhere else, a handful a cell
    lens1 = rng.randint(0, 5, D).astype(np.int64)
    off = [np.concatenate([[0], np.cumsum(lens0)]), np.concatenate([[0], np.cumsum(lens1)])]
    t1 = rng.randint(0, V[1], off[1][-1]).astype(np.int32)
    z1 = rng.randint(0, K, off[1][-1]).astype(np.int32)
    return Corpus(K, V, off, [types, t1]), [z, z1]


def pair(K, seed):
    c, z0 = corpus_with_every_row_class(K, seed)
    hy = Hyper.defaults(K, c.V)
    o = make_oracle(c, hy)
    for m in range(c.M):
        o.set_assignments(m, z0[m])
    o.build_counts()
    return c, hy, o, z0


def oracle_segmented(o, c, it, seed, nseg):
    """tests/test_gpu_segmented.py::oracle_segmented_sweep without topic births, which also returns the counts the LAST segment started
    from: what the library's last rebuild of the sweep classed the rows by and wrote the image from"""
    from oracle.binding import SWEEP_NO_APPLY as ORC_NO_APPLY
    stats = dict(tokens=0, changed=0, new_mass_cnt=0, topic_doc_mass_cnt=0, word_ftree_mass_cnt=0)
    for docs in segment_lists(c, nseg):
        before = np.concatenate([o.get_counts(m)[0] for m in range(c.M)])
        r = o.sweep_list(it, seed, docs, flags=ORC_NO_APPLY, want_delta=True)
        st = r["stats"]
        o.apply_delta(r["delta_nwk"], r["delta_nk"], st["activated_topic"], st["activated_modality"])
        for k in stats:
            stats[k] += st[k]
    return stats, before


def device_bytes(s, which):
    import torch
    from mvtopicmodel_amd.dist import _DevArray
    ptr, n = s.device_buffer(which)
    s.synchronize()
    return torch.as_tensor(_DevArray(ptr, n, "|u1"), device="cuda:0")


def unpack12(rows, K):
    """[n][128 * ceil(K / 85)] bytes -> [n][K] cells, by the definition of the layout"""
    k = np.arange(K)
    byte = 128 * (k // 85) + ((3 * (k % 85)) >> 1)
    shift = 4 * ((k % 85) & 1)
    u16 = rows[:, byte].astype(np.uint32) | (rows[:, byte + 1].astype(np.uint32) << 8)
    return ((u16 >> shift) & 0xfff).astype(np.int32)


def check_image_against(s, nwk_all, K):
    """the row classes and the image as the last tree build left them, against the counts it was built from"""
    cls = device_bytes(s, BUF_ROW_CLASS).cpu().numpy()
    tot, big = nwk_all.sum(axis=1), nwk_all.max(axis=1)
    assert np.array_equal(cls & 3, np.where(tot > 65534, 1, np.where(tot > 32767, 2, 0)))
    assert np.array_equal((cls & ROW_SLIM) != 0, big <= 4095)
    stride = 128 * ((K + 84) // 85)
    img = device_bytes(s, BUF_COUNTS12).cpu().numpy().reshape(-1, stride)
    slim = big <= 4095
    assert np.array_equal(unpack12(img[slim], K), nwk_all[slim])
    return slim


@pytest.mark.parametrize("force", [0, 1, 2, 4])       # 0: every entity on the narrowest variant that holds its list; R: nothing narrower than R rounds
# K: 4 lines to the last cell, 5 lines with one cell in the last, 6 lines; 600 and 1000: 8 and 12 lines, and the 2-round variant in its build for
# rows of 1 KiB and more (K >= 512: the one C5 runs)
@pytest.mark.parametrize("K", [340, 341, 426, 600, 1000])
def test_three_way_gather_is_the_oracles_sweep_with_the_table_and_without(monkeypatch, K, force):
    c, hy, o, z0 = pair(K, 100 + K)
    monkeypatch.delenv("MVHDP_SLIM", raising=False)
    s_on = make_native(c, hy, z0)
    monkeypatch.setenv("MVHDP_SLIM", "0")
    s_off = make_native(c, hy, z0)
    monkeypatch.delenv("MVHDP_SLIM")
    assert s_on.device_buffer(BUF_COUNTS12)[1] == (c.V[0] + c.V[1]) * 128 * ((K + 84) // 85)
    with pytest.raises(MvhdpError):
        s_off.device_buffer(BUF_COUNTS12)
    for s in (s_on, s_off):
        s.set_tuning(walk_fixed=1, walk_theta=[0.3, 0.3], **({"force_primary": force} if force else {}))
    nwk0 = o.get_counts(0)[0]
    assert nwk0[0].max() > 65534 and nwk0[1].max() == 4095 and nwk0[2].max() == 4096
    assert nwk0[3].sum() > 32767 and nwk0[3].max() <= 4095 and nwk0[4].sum() > 65534 and nwk0[4].max() <= 4095
    slim_seen = []
    for it in range(5):
        before = np.concatenate([o.get_counts(m)[0] for m in range(c.M)])
        if it < 3:
            ro = o.sweep(it, 77)["stats"]
            flags = 0
        else:                                                            # rows are classed again at each segment's rebuild
            ro, before = oracle_segmented(o, c, it, 77, 3)
            flags = SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(3)
        for name, s in (("table", s_on), ("switch off", s_off)):
            rs = s.sweep(it, 77, flags=flags)
            for f in STATS:
                if f in ro:
                    assert ro[f] == getattr(rs, f), (name, it, f)
            assert_same_state(o, s, c.M)
        slim = check_image_against(s_on, before, K)                      # (a segmented sweep: as its last segment's rebuild left them)
        if it < 3:
            slim_seen.append(slim)
    # the three classes in one view, and rows that moved between them from one sweep to the next
    assert slim_seen[0][1] and not slim_seen[0][2] and not slim_seen[0][0] and slim_seen[0][3] and slim_seen[0][4]
    assert any((a != b).any() for a, b in zip(slim_seen, slim_seen[1:])), "no row changed class between sweeps"
    s_on.close(); s_off.close()


def test_the_kernel_really_reads_the_image():
    """Trees built, then the image of ONE slim word doctored behind the library's back (values that fit 12 bits, in place): a sweep
    that re-uses those trees must part from the oracle's, and only in entities that hold that word (a deferred sweep reads nothing
    else that another entity wrote)."""
    K = 340
    c, hy, o, z0 = pair(K, 7)
    s = make_native(c, hy, z0)
    s.set_tuning(walk_fixed=1, walk_theta=[0.3, 0.3])
    s.build_trees()
    img = device_bytes(s, BUF_COUNTS12)
    cls = device_bytes(s, BUF_ROW_CLASS).cpu().numpy()
    assert cls[3] & ROW_SLIM
    stride = 128 * ((K + 84) // 85)
    row = img[3 * stride:4 * stride].cpu().numpy()
    assert np.array_equal(unpack12(row[None, :], K)[0], o.get_counts(0)[0][3])
    import torch
    img[3 * stride:4 * stride] = torch.zeros(stride, dtype=torch.uint8, device="cuda:0")      # word 3: every count reads 0
    torch.cuda.synchronize()
    rs = s.sweep(0, 5, flags=SWEEP_REUSE_TREES)
    ro = o.sweep(0, 5)["stats"]
    zo, zs = o.get_assignments(0), s.get_assignments(0)
    differ = zo != zs
    assert differ.any(), "the sweep did not read the 12-bit image"
    assert rs.tokens == ro["tokens"]
    # only entities that hold word 3 can have seen anything else than the oracle saw
    ents = np.unique(np.searchsorted(c.doc_off[0], np.flatnonzero(differ), side="right") - 1)
    has3 = np.array([np.any(c.tokens[0][c.doc_off[0][d]:c.doc_off[0][d + 1]] == 3) for d in ents])
    assert has3.all()
    s.close()
