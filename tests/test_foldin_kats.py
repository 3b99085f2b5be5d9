"""mvhdp_fold_in without a device: the entry through every layer (header, loader, library export, wrappers, build list, documents), and the
sequential restatement of its contract (tests/native/foldin_ref.c) against known answers worked here from the header's formulas, against
the exact distribution of a one-token document, and against the properties the header guarantees."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from tests import foldin_cases as fc
from tests import foldin_ref as fr
from tests.ltr_cases import lane_order_total

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_FIELDS = ["iterations", "samples", "thin", "seed", "doc_base", "coupling", "view_weights"]
STATS_FIELDS = ["tokens", "oov", "visits", "kernel_ms"]
WRAPPER = ["self", "doc_off", "tokens", "view_weights", "iterations", "samples", "thin", "seed", "doc_base", "coupling", "want_z", "want_counts"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_exists_in_every_layer():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mvhdp_fold_in\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_foldin_args\s*\*", code)
    for name, fields in (("mvhdp_foldin_args", ARGS_FIELDS), ("mvhdp_foldin_stats", STATS_FIELDS)):
        st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
        assert st and [f.split()[-1].lstrip("*") for f in re.split(r"[;,]", st.group(1)) if f.strip()] == fields, name
    for phrase in ("foldin_ref.c", "base_m[k] = a_m[k] + o_m[k]", "it + m * 2^16", "Departures from the frozen-sweep inferencer"):
        assert phrase in hdr, phrase
    from mvtopicmodel_amd import _lib, native
    assert "mvhdp_fold_in" in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.FoldinArgsC._fields_] == ARGS_FIELDS and C.sizeof(_lib.FoldinArgsC) == 48
    assert [f[0] for f in _lib.FoldinStatsC._fields_] == STATS_FIELDS and C.sizeof(_lib.FoldinStatsC) == 32
    L = _lib.load_library()
    assert len(L.mvhdp_fold_in.argtypes) == 9 and L.mvhdp_fold_in.restype is C.c_int
    assert L.mvhdp_fold_in(None, None, 0, None, None, None, None, None, None) == -1      # a NULL handle: no device touched
    for cls in (native.NativeSampler, native.NativeGroup):
        sig = inspect.signature(cls.fold_in).parameters
        assert list(sig) == WRAPPER
        assert [sig[n].default for n in WRAPPER[4:]] == [10, 1, 1, 0, 0, None, False, False]
    assert [f.name for f in native.FoldinResult.__dataclass_fields__.values()] == ["theta", "z", "counts_sum", "tokens", "oov", "visits", "kernel_ms"]
    assert "mvhdp_foldin.hip" in re.search(r"^SRCS\s*=(.*)$", read("mvtopicmodel_amd", "csrc", "Makefile"), flags=re.M).group(1)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "CHANGELOG.md"):
        assert "mvhdp_fold_in" in read(doc), doc
    assert "Not done: a JNI class" in read("README.md")
    assert "nearest_entities(" in read("INTEGRATION.md") and "fold_in(" in read("INTEGRATION.md")


def running_sums_T1(wt):
    """K <= 3, T = 1: the running sum at topic k is excl(k) + wt[k]; excl(1) = wt[0], excl(2) = wt[1] + wt[0] (lane 1 after the scan's first step)"""
    return [0.0 + wt[0], wt[0] + wt[1], (wt[1] + wt[0]) + wt[2]]


def draw_T1(wt, u, total):
    run = running_sums_T1(wt)
    for k in range(3):
        if wt[k] > 0.0 and run[k] > u * total:
            return k
    return max(k for k in range(3) if wt[k] > 0.0)


def test_known_answer_one_view_two_tokens():
    nwk = np.array([[7, 1, 2], [0, 9, 4]], dtype=np.int32)
    nk = np.array([40, 35, 20], dtype=np.int32)
    beta, beta_sum, gamma, alpha_sum = 0.01, 0.02, 0.85, 0.4
    alpha = np.array([0.1, 0.07, 0.12])
    mdl = fr.Model([nwk], nk[None, :], np.array([beta]), np.array([beta_sum]), np.array([gamma]), alpha[None, :], np.array([alpha_sum]),
                   None, np.array([[0.2]]), np.array([[1.0]]))
    seed, base = (5 << 32) | 77, (3 << 32) | 9
    got = fr.run(mdl, [np.array([0, 2])], [np.array([0, 1])], view_weights=[1.0], iterations=1, seed=seed, doc_base=base, trace=True)
    # by hand: a = gamma * alpha; no other view, so s = 0.0, o = 0.0 * Lp, base = a + o
    Lp = 2.0 + gamma * alpha_sum
    a = [gamma * float(x) for x in alpha]
    basev = [a[k] + 0.0 * Lp for k in range(3)]
    rinv = [1.0 / (float(nk[k]) + beta_sum) for k in range(3)]
    n = [0, 0, 0]
    zs = []
    for pos, w in enumerate([0, 1]):
        wt = [(1.0 * float(n[k]) + basev[k]) * ((float(nwk[w][k]) + beta) * rinv[k]) for k in range(3)]
        total = lane_order_total(wt)
        u = fr.unit([9, 3, 1 + (0 << 16), pos], [77, 5])
        assert 0.0 <= u < 1.0
        row = got.trace_wt[pos]
        assert row[0] == total and row[1] == u and list(row[2:]) == wt, (pos, row, total, wt)
        z = draw_T1(wt, u, total)
        zs.append(z)
        n[z] += 1
    assert list(got.z[0]) == zs
    assert list(got.counts_sum[0, 0]) == n and (got.tokens, got.oov, got.visits) == (2, 0, 2)
    theta = [(1.0 * ((float(n[k]) / 1.0 + a[k]) / Lp)) / 1.0 for k in range(3)]
    assert list(got.theta[0]) == [0.0 + t for t in theta]


def test_known_answer_base_of_the_second_view():
    mdl = fc.random_model(2, [5, 4], seed=4)
    P = np.array([[1.0, 0.3], [0.45, 0.8]])
    off = [np.array([0, 3]), np.array([0, 2])]
    tok = [np.array([1, 4, 0]), np.array([3, 3])]
    got = fr.run(mdl, off, tok, iterations=1, seed=2, coupling=P, trace=True)
    ndk0 = np.bincount(got.z[0], minlength=2).astype(np.float64)
    a0, a1 = mdl.gamma[0] * mdl.alpha[0], mdl.gamma[1] * mdl.alpha[1]
    Lp0, Lp1 = 3.0 + mdl.gamma[0] * mdl.alpha_sum[0], 2.0 + mdl.gamma[1] * mdl.alpha_sum[1]
    s = 0.0 + P[1, 0] * (ndk0 + a0) / Lp0                                    # WRK:404: product, then quotient, added from 0.0
    base1 = a1 + s * Lp1                                                     # WRK:409 and the gamma * alpha term
    assert np.array_equal(got.trace_base[0, 1], base1)
    s0 = 0.0 + P[0, 1] * (np.zeros(2) + a1) / Lp1                            # view 0 goes first: view 1 holds nothing yet
    assert np.array_equal(got.trace_base[0, 0], a0 + s0 * Lp0)


def test_one_token_documents_follow_the_exact_distribution():
    p, half, prior = fc.peaked_expectation()
    off, tok = fc.peaked_docs()
    got = fr.run(fc.peaked_model(), off, tok, iterations=1, seed=11, doc_base=1000)
    freq = fc.frequencies(got.z[0])
    print("frequencies", freq, "exact", p, "half-widths", half)
    assert (np.abs(freq - p) <= half).all()
    assert (np.abs(prior - p) > half).any() and not (np.abs(freq - prior) <= half).all()   # the prior alone is another distribution


def test_properties_of_the_restatement():
    K, V = 6, [20, 9, 7]
    inactive = np.array([0, 0, 1, 0, 0, 1], dtype=np.uint8)
    mdl = fc.random_model(K, V, seed=1, inactive=inactive)
    offs, toks = fc.foldin_docs(V, n_docs=24, seed=3, lengths=[0, 1, 2, 9, 17])
    w = [1.0, 0.5, 0.25]
    whole = fr.run(mdl, offs, toks, w, iterations=4, seed=6, doc_base=50)
    assert whole.oov > 0 and whole.visits == 4 * whole.tokens
    for m in range(3):
        z, t = whole.z[m], toks[m]
        assert ((z == -1) == (t >= V[m])).all()                              # every in-vocabulary token is assigned, no other
        assert not np.isin(z, [2, 5]).any()                                  # an inactive topic is never drawn
        for d in range(24):                                                  # S = 1: counts_sum is the recount of z
            zz = z[offs[m][d]:offs[m][d + 1]]
            assert np.array_equal(whole.counts_sum[d, m], np.bincount(zz[zz >= 0], minlength=K))
    assert np.allclose(whole.theta.sum(1), [sum(w[m] * (mdl.gamma[m] * mdl.alpha[m].sum() + (whole.z[m][offs[m][d]:offs[m][d + 1]] >= 0).sum())
                                                / (offs[m][d + 1] - offs[m][d] + mdl.gamma[m] * mdl.alpha_sum[m]) for m in range(3)) / sum(w) for d in range(24)])
    # a batch split in two calls with shifted doc_base gives the same rows
    a = 10
    for part, lo, hi in ((fr.run(mdl, *fc.slice_docs(offs, toks, 0, a), w, iterations=4, seed=6, doc_base=50), 0, a),
                         (fr.run(mdl, *fc.slice_docs(offs, toks, a, 24), w, iterations=4, seed=6, doc_base=50 + a), a, 24)):
        assert part.theta.tobytes() == whole.theta[lo:hi].tobytes() and np.array_equal(part.counts_sum, whole.counts_sum[lo:hi])
        for m in range(3):
            assert np.array_equal(part.z[m], whole.z[m][offs[m][lo]:offs[m][hi]])
    # samples: the sum of S recorded states holds S times the assigned tokens, and S = 1 at the same iteration is one of them
    s3 = fr.run(mdl, offs, toks, w, iterations=7, samples=3, thin=2, seed=6)
    s1 = fr.run(mdl, offs, toks, w, iterations=7, seed=6)
    assert np.array_equal(s3.counts_sum.sum(2), 3 * s1.counts_sum.sum(2)) and (s3.counts_sum >= s1.counts_sum).all()
    for m in range(3):
        assert np.array_equal(s3.z[m], s1.z[m])
    # another seed is another chain; a zero coupling row cuts a view off from the others
    assert fr.run(mdl, offs, toks, w, iterations=4, seed=7, doc_base=50).theta.tobytes() != whole.theta.tobytes()
    cut = fr.run(mdl, offs, toks, iterations=2, seed=6, coupling=np.eye(3))
    alone = fr.run(mdl, [offs[0], None, None], [toks[0], None, None], iterations=2, seed=6, coupling=np.eye(3))
    assert np.array_equal(cut.z[0], alone.z[0])
