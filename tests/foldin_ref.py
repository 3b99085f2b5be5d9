"""ctypes wrapper of tests/native/foldin_ref.c, the sequential restatement of mvhdp_fold_in as include/mvhdp.h defines it (built once per
process with gcc -O2 -ffp-contract=off into a temporary directory).  Test infrastructure: no GPU, no product code."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests.native_build import ptr, ptr_array, ref_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("foldin_ref")
        vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
        L.foldin_run.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, u64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.foldin_run.restype = i32
        L.foldin_philox.argtypes = [vp, vp, vp]
        L.foldin_unit.argtypes = [C.c_uint32, C.c_uint32]
        L.foldin_unit.restype = C.c_double
        _lib = L
    return _lib


@dataclass
class Model:
    """the frozen model a fold-in reads: per view n_wk [V_m][K] and n_k [K]; beta, beta_sum, gamma, alpha_sum [M]; alpha [M][K];
    inactive [K] or None; p_a, p_b [M][M] (the default coupling's source)"""
    nwk: list
    nk: np.ndarray
    beta: np.ndarray
    beta_sum: np.ndarray
    gamma: np.ndarray
    alpha: np.ndarray
    alpha_sum: np.ndarray
    inactive: np.ndarray = None
    p_a: np.ndarray = None
    p_b: np.ndarray = None

    @property
    def M(self):
        return len(self.nwk)

    @property
    def K(self):
        return self.nwk[0].shape[1]


def default_coupling(p_a, p_b, M):
    """the header's P for args.coupling == NULL"""
    P = np.zeros((M, M))
    for m in range(M):
        for i in range(M):
            if i == m:
                P[m, i] = 1.0
            elif p_a[m][i] != 0.0:
                P[m, i] = p_a[m][i] / (p_a[m][i] + p_b[m][i])
    return P


@dataclass
class Ref:
    theta: np.ndarray
    z: list
    counts_sum: np.ndarray
    tokens: int
    oov: int
    visits: int
    trace_wt: np.ndarray = None        # one document: per visit total, u, wt[0..K)
    trace_base: np.ndarray = None      # one document: [iterations][M][K]


def run(model, doc_off, tokens, view_weights=None, iterations=10, samples=1, thin=1, seed=0, doc_base=0, coupling=None, trace=False):
    M, K = model.M, model.K
    nwk = [np.ascontiguousarray(x, dtype=np.int32) for x in model.nwk]
    V = np.array([x.shape[0] for x in nwk], dtype=np.int32)
    nk = np.ascontiguousarray(model.nk, dtype=np.int32).reshape(M, K)
    dbl = lambda x, shape: np.ascontiguousarray(np.asarray(x, dtype=np.float64)[tuple(slice(0, s) for s in shape)])
    beta, beta_sum, gamma, alpha_sum = (dbl(x, (M,)) for x in (model.beta, model.beta_sum, model.gamma, model.alpha_sum))
    alpha = dbl(model.alpha, (M, K))
    inactive = None if model.inactive is None else np.ascontiguousarray(model.inactive, dtype=np.uint8)
    P = dbl(coupling, (M, M)) if coupling is not None else default_coupling(model.p_a, model.p_b, M)
    offs = [None if o is None else np.ascontiguousarray(o, dtype=np.int64) for o in doc_off]
    toks = [None if o is None else np.ascontiguousarray(t if t is not None else [], dtype=np.int32) for o, t in zip(offs, tokens)]
    D = max([len(o) - 1 for o in offs if o is not None], default=0)
    for o, t in zip(offs, toks):
        assert o is None or (len(o) - 1 == D and o[0] == 0 and len(t) == o[-1] and (t >= 0).all())
    w = None if view_weights is None else dbl(view_weights, (M,))
    theta = np.zeros((D, K)) if w is not None else None
    z = [None if o is None else np.full(len(t), -1, dtype=np.int32) for o, t in zip(offs, toks)]
    cs = np.zeros((D, M, K), dtype=np.int32)
    totals = np.zeros(3, dtype=np.int64)
    n_in = sum(int((t < v).sum()) for t, v in zip(toks, V) if t is not None)
    tw = np.zeros((n_in * iterations, K + 2)) if trace else None
    tb = np.zeros((iterations, M, K)) if trace else None
    keep = (ptr_array(nwk), ptr_array(offs), ptr_array(toks), ptr_array(z))
    rc = lib().foldin_run(K, M, ptr(V), keep[0], ptr(nk), ptr(beta), ptr(beta_sum), ptr(gamma), ptr(alpha), ptr(alpha_sum), ptr(inactive), ptr(P),
                          int(iterations), int(samples), int(thin), int(seed), int(doc_base), D, keep[1], keep[2], ptr(w), ptr(theta), keep[3], ptr(cs),
                          ptr(totals), ptr(tw), ptr(tb))
    assert rc == 0, rc
    return Ref(theta, z, cs, int(totals[0]), int(totals[1]), int(totals[2]), tw, tb)


def philox(ctr, key):
    c = np.array(ctr, dtype=np.uint32); k = np.array(key, dtype=np.uint32); o = np.zeros(4, dtype=np.uint32)
    lib().foldin_philox(ptr(c), ptr(k), ptr(o))
    return [int(x) for x in o]


def unit(ctr, key):
    """u of the header's draw for a counter (document low, document high, it + m * 2^16, pos) and key (seed low, seed high)"""
    x = philox(ctr, key)
    return float(lib().foldin_unit(x[0], x[1]))
