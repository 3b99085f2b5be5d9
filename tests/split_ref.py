"""ctypes wrapper of tests/native/split_ref.c, the sequential restatement of mvhdp_split_topic as include/mvhdp.h defines it (built once
per process with gcc -O2 -ffp-contract=off into a temporary directory).  Test infrastructure: no GPU, no product code."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests.foldin_ref import default_coupling
from tests.native_build import ptr, ptr_array, ref_lib

KEEP_ALPHA = 0x1
MAXM = 8
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("split_ref")
        vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
        L.split_run.argtypes = [i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, u32, u64, i64, vp, vp, vp, vp, i64, vp]
        L.split_run.restype = i32
        L.split_philox.argtypes = [vp, vp, vp]
        L.split_unit.argtypes = [u32, u32]
        L.split_unit.restype = C.c_double
        _lib = L
    return _lib


def counts_of(K, V, tokens, z):
    """(n_wk [V][K], n_k [K]) of one view's assignments, unassigned tokens in no count"""
    nwk = np.zeros((V, K), dtype=np.int32)
    on = z >= 0
    np.add.at(nwk, (tokens[on], z[on]), 1)
    return nwk, nwk.sum(0).astype(np.int32)


@dataclass
class Ref:
    rc: int
    z: list = None
    alpha: np.ndarray = None
    inactive: np.ndarray = None
    split: np.ndarray = None
    moved: np.ndarray = None
    flips_last: int = 0
    target: int = -1
    activated: int = 0
    flips: np.ndarray = None
    trace: np.ndarray = None           # [visits][4]: u, wt[a], wt[b], total


def run(K, V, doc_off, tokens, z, hy, source, target=None, iterations=20, seed=0, coupling=None, type_hint=None, keep_alpha=False,
        doc_id_base=0, flags=None, trace=False, nk=None):
    """z' , alpha', inactive', the statistics and flips of a split of `source` on the state (z, hy); hy: a native.Hyper.  rc != 0: refused,
    nothing else is set."""
    M = len(V)
    Vv = np.array(V, dtype=np.int32)
    offs = [np.ascontiguousarray(o, dtype=np.int64) for o in doc_off]
    toks = [np.ascontiguousarray(t, dtype=np.int32) for t in tokens]
    zz = [np.array(x, dtype=np.int32) for x in z]
    D = len(offs[0]) - 1
    if nk is None:                                           # n_k [M][K] of z (a caller that holds the counts may pass them)
        nk = np.stack([counts_of(K, V[m], toks[m], zz[m])[1] for m in range(M)])
    nk = np.ascontiguousarray(nk, dtype=np.int32).reshape(M, K)
    dbl = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:M])
    beta, beta_sum, gamma, alpha_sum = dbl(hy.beta), dbl(hy.beta_sum), dbl(hy.gamma), dbl(hy.alpha_sum)
    alpha = np.array(np.asarray(hy.alpha, dtype=np.float64)[:M, :K + 1])
    inactive = np.zeros(K, dtype=np.uint8) if hy.inactive is None else np.array(hy.inactive, dtype=np.uint8)
    P = np.ascontiguousarray(coupling, dtype=np.float64).reshape(M, M) if coupling is not None else default_coupling(hy.p_a, hy.p_b, M)
    hints = None
    if type_hint is not None:
        hints = [None if r is None else np.ascontiguousarray(r, dtype=np.int8) for r in type_hint]
        assert len(hints) == M and all(r is None or r.shape == (V[m],) for m, r in enumerate(hints))
    stats = np.zeros(2 * MAXM + 3, dtype=np.int64)
    flips = np.zeros(max(int(iterations), 1), dtype=np.int64)
    n_set = sum(int((zz[m] == source).sum()) for m in range(M))
    cap = n_set * max(int(iterations), 0) if trace else 0
    tr = np.zeros((max(cap, 1), 4)) if trace else None
    ntr = np.zeros(1, dtype=np.int64)
    keep = (ptr_array(offs), ptr_array(toks), ptr_array(zz), None if hints is None else ptr_array(hints))
    fl = (KEEP_ALPHA if keep_alpha else 0) if flags is None else flags
    rc = lib().split_run(K, M, ptr(Vv), D, keep[0], keep[1], keep[2], ptr(nk), ptr(beta), ptr(beta_sum), ptr(gamma), ptr(alpha), ptr(alpha_sum),
                         ptr(inactive), ptr(P), int(source), -1 if target is None else int(target), int(iterations), fl, int(seed),
                         int(doc_id_base), keep[3], ptr(stats), ptr(flips), ptr(tr), cap, ptr(ntr))
    if rc != 0:
        return Ref(rc)
    return Ref(0, zz, alpha, inactive, stats[:M].copy(), stats[MAXM:MAXM + M].copy(), int(stats[2 * MAXM]), int(stats[2 * MAXM + 1]),
               int(stats[2 * MAXM + 2]), flips[:max(int(iterations), 0)].copy(), None if tr is None else tr[:int(ntr[0])])


def philox(ctr, key):
    c = np.array(ctr, dtype=np.uint32); k = np.array(key, dtype=np.uint32); o = np.zeros(4, dtype=np.uint32)
    lib().split_philox(ptr(c), ptr(k), ptr(o))
    return [int(x) for x in o]


def unit(g, it, m, pos, seed):
    """u of the header's draw for entity g (global id), iteration it, view m, position pos inside the span"""
    x = philox([g & 0xFFFFFFFF, g >> 32, it + (m << 16), pos], [seed & 0xFFFFFFFF, seed >> 32])
    return float(lib().split_unit(x[0], x[1]))
