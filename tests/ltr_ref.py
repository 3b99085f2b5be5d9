"""ctypes wrapper of tests/native/ltr_ref.c, the sequential restatement of the left-to-right held-out estimator of include/mvhdp.h
(built once per process with gcc -O2 -ffp-contract=off into a temporary directory), and the numpy side of the per-document logs.  Test
infrastructure: no GPU, no product code."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from tests.native_build import ptr, ref_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("ltr_ref")
        vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
        L.ltr_evaluate.argtypes = [i32, i32, vp, vp, dbl, vp, dbl, i32, i32, u64, i64, i64, vp, vp, vp, vp, vp, vp]
        L.ltr_evaluate.restype = i32
        L.ltr_philox.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


@dataclass
class Ref:
    S: np.ndarray              # [N] sum over particles of p_r[n]; 0 at an out-of-vocabulary position
    P: np.ndarray              # [R][N] p_r[n], or None
    doc_tokens: np.ndarray     # [D]
    tokens: int
    oov: int
    visits: int
    doc_ll: np.ndarray         # [D] numpy's logs of S, summed exactly (math.fsum)
    doc_bound: np.ndarray      # [D] 8 * 2^-53 * sum_n (|log S[n]| + log R)
    log_likelihood: float
    bound: float


def doc_logs(S, doc_off, R):
    """per document: fsum over S[n] > 0 of (log S[n] - log R), and the bound 8 * 2^-53 * sum (|log S[n]| + log R) a device sum of the same S may
    differ by (its log is not glibc's: two ulp per term, plus the summation)"""
    D = len(doc_off) - 1
    ll, bound = np.zeros(D), np.zeros(D)
    log_r = math.log(R)
    for d in range(D):
        s = S[doc_off[d]:doc_off[d + 1]]
        lg = np.log(s[s > 0])
        ll[d] = math.fsum(float(x) - log_r for x in lg)
        bound[d] = 8 * 2.0 ** -53 * math.fsum(abs(float(x)) + log_r for x in lg)
    return ll, bound


def evaluate(nwk, nk, beta, alpha, alpha_sum, doc_off, tok, particles=10, resample=True, seed=0, doc_base=0, want_P=False):
    """nwk [V][K], nk [K] of one view; alpha [K] as used (alpha_k), alpha_sum = alphaSum'"""
    nwk = np.ascontiguousarray(nwk, dtype=np.int32)
    nk = np.ascontiguousarray(nk, dtype=np.int32)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    tok = np.ascontiguousarray(tok, dtype=np.int32)
    V, K = nwk.shape
    assert nk.shape == (K,) and alpha.shape == (K,) and len(tok) == doc_off[-1] and doc_off[0] == 0 and (tok >= 0).all()
    D, N = len(doc_off) - 1, len(tok)
    S = np.zeros(N)
    P = np.zeros((particles, N)) if want_P else None
    doc_tokens = np.zeros(D, dtype=np.int64)
    totals = np.zeros(3, dtype=np.int64)
    rc = lib().ltr_evaluate(K, V, ptr(nwk), ptr(nk), float(beta), ptr(alpha), float(alpha_sum), int(particles), 1 if resample else 0, int(seed), int(doc_base),
                            D, ptr(doc_off), ptr(tok), ptr(S), ptr(P), ptr(doc_tokens), ptr(totals))
    assert rc == 0
    ll, bound = doc_logs(S, doc_off, particles)
    total = 0.0
    for x in ll:
        total += float(x)
    return Ref(S, P, doc_tokens, int(totals[0]), int(totals[1]), int(totals[2]), ll, bound, total, float(bound.sum()))


def philox(ctr, key):
    c = np.array(ctr, dtype=np.uint32); k = np.array(key, dtype=np.uint32); o = np.zeros(4, dtype=np.uint32)
    lib().ltr_philox(ptr(c), ptr(k), ptr(o))
    return [int(x) for x in o]
