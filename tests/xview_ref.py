"""ctypes wrapper of tests/native/xview_ref.c, the sequential restatement of the cross-view prediction contract of include/mvhdp.h
(built once per process with gcc -O2 -ffp-contract=off into a temporary directory).  Test infrastructure: no GPU, no product code."""
import ctypes as C

import numpy as np

from tests.native_build import ptr, ref_lib

ASCENDING, DESCENDING, UNFUSED = 0, 1, 2         # xview_chain's variants: the contract's chain, and two the sensitivity tests run
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("xview_ref")
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.xview_chain.argtypes = [i32, vp, vp, i32]
        L.xview_chain.restype = dbl
        L.xview_phi.argtypes = [i32, i32, vp, vp, vp, dbl, dbl, vp]
        L.xview_phi.restype = None
        L.xview_scores.argtypes = [i32, i32, i64, vp, vp, i32, vp]
        L.xview_scores.restype = None
        L.xview_predict.argtypes = [i32, i64, vp, i32, vp, vp, i32, vp, vp, vp]
        L.xview_predict.restype = i32
        L.xview_score_pairs.argtypes = [i32, vp, i32, vp, vp, i64, vp, vp, vp, vp]
        L.xview_score_pairs.restype = i32
        _lib = L
    return _lib


def chain(theta, phi, variant=ASCENDING):
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    assert theta.shape == phi.shape and theta.ndim == 1
    return float(lib().xview_chain(len(theta), ptr(theta), ptr(phi), int(variant)))


def phi_table(nwk, nk, beta, beta_sum, inactive=None):
    nwk = np.ascontiguousarray(nwk, dtype=np.int32)
    nk = np.ascontiguousarray(nk, dtype=np.int32)
    V, K = nwk.shape
    assert nk.shape == (K,)
    ina = None if inactive is None else np.ascontiguousarray(inactive, dtype=np.uint8)
    out = np.zeros((V, K))
    lib().xview_phi(K, V, ptr(nwk), ptr(nk), ptr(ina), float(beta), float(beta_sum), ptr(out))
    return out


def scores(theta, phi, variant=ASCENDING):
    """[D][V]: every entity against every type"""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    D, K = theta.shape
    V = phi.shape[0]
    assert phi.shape == (V, K)
    out = np.zeros((D, V))
    lib().xview_scores(K, V, D, ptr(theta), ptr(phi), int(variant), ptr(out))
    return out


def _span(D, doc_off, tok):
    if doc_off is None:
        return np.zeros(D + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    tok = np.ascontiguousarray(tok, dtype=np.int32)
    assert len(doc_off) == D + 1 and len(tok) == doc_off[-1]
    return doc_off, tok


def predict(S, n, exclude_present=False, doc_off=None, tok=None):
    """S [D][V] scores; doc_off / tok: the view's spans of the same entities -> (items [D][n], scores [D][n], counts [D])"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    D, V = S.shape
    doc_off, tok = _span(D, doc_off, tok)
    items = np.zeros((D, n), dtype=np.int32)
    sc = np.zeros((D, n))
    counts = np.zeros(D, dtype=np.int32)
    assert lib().xview_predict(V, D, ptr(S), 1 if exclude_present else 0, ptr(doc_off), ptr(tok), int(n), ptr(items), ptr(sc), ptr(counts)) == 0
    return items, sc, counts


def score_pairs(S, entity, item, exclude_present=False, doc_off=None, tok=None):
    """entity: row indices of S -> (score [P], rank [P])"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    D, V = S.shape
    doc_off, tok = _span(D, doc_off, tok)
    entity = np.ascontiguousarray(entity, dtype=np.int64)
    item = np.ascontiguousarray(item, dtype=np.int32)
    assert entity.shape == item.shape and (len(entity) == 0 or (entity.min() >= 0 and entity.max() < D and item.min() >= 0 and item.max() < V))
    score = np.zeros(len(entity))
    rank = np.zeros(len(entity), dtype=np.int32)
    assert lib().xview_score_pairs(V, ptr(S), 1 if exclude_present else 0, ptr(doc_off), ptr(tok), len(entity), ptr(entity), ptr(item), ptr(score), ptr(rank)) == 0
    return score, rank
