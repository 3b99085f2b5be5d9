"""ctypes wrapper of tests/native/xview_entities_ref.c, the sequential restatement of the entities-for-an-item contract of include/mvhdp.h
(built once per process with gcc -O2 -ffp-contract=off, together with tests/native/xview_ref.c whose xview_phi it calls, into a temporary
directory).  Test infrastructure: no GPU, no product code."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests.native_build import ptr, ref_lib

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("xview_entities_ref", "xview_ref.c")
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.xve_psi_from_counts.argtypes = [i32, i32, vp, vp, vp, dbl, dbl, i64, vp, vp, vp, vp]
        L.xve_psi_from_counts.restype = i32
        L.xve_scores.argtypes = [i32, i64, i64, vp, vp, vp]
        L.xve_scores.restype = None
        L.xve_excluded.argtypes = [i64, vp, vp, i64, vp, vp, vp]
        L.xve_excluded.restype = None
        L.xve_predict.argtypes = [i64, i64, vp, vp, i32, i64, vp, vp, vp]
        L.xve_predict.restype = i32
        L.xve_rank.argtypes = [i64, vp, vp, i64, vp, vp, vp, vp]
        L.xve_rank.restype = None
        _lib = L
    return _lib


def flatten(items, weights=None):
    """a list of lists (or a 1-D array: one item per query) -> (q_off [nq+1] int64, q_items int32, q_weights float64 or None)"""
    if isinstance(items, np.ndarray) and items.ndim == 1:
        items = [[int(i)] for i in items]
        weights = None if weights is None else [[float(x)] for x in weights]
    off = np.concatenate([[0], np.cumsum([len(q) for q in items])]).astype(np.int64)
    flat = np.array([i for q in items for i in q], dtype=np.int32)
    fw = None if weights is None else np.array([x for q in weights for x in q], dtype=np.float64)
    assert fw is None or len(fw) == len(flat)
    return off, flat, fw


def psi_rows(nwk, nk, beta, beta_sum, inactive, items, weights=None):
    """[nq][K]: the query rows from the count table"""
    nwk = np.ascontiguousarray(nwk, dtype=np.int32)
    nk = np.ascontiguousarray(nk, dtype=np.int32)
    V, K = nwk.shape
    ina = None if inactive is None else np.ascontiguousarray(inactive, dtype=np.uint8)
    off, flat, fw = flatten(items, weights)
    assert len(flat) == 0 or (flat.min() >= 0 and flat.max() < V)
    out = np.zeros((len(off) - 1, K))
    assert lib().xve_psi_from_counts(K, V, ptr(nwk), ptr(nk), ptr(ina), float(beta), float(beta_sum), len(off) - 1, ptr(off), ptr(flat), ptr(fw), ptr(out)) == 0
    return out


def scores(theta, psi):
    """[nq][C]: every query against every candidate row of theta"""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    Cn, K = theta.shape
    nq = psi.shape[0]
    assert psi.shape == (nq, K)
    out = np.zeros((nq, Cn))
    lib().xve_scores(K, nq, Cn, ptr(theta), ptr(psi), ptr(out))
    return out


def excluded(doc_off, tok, items):
    """[nq][C] uint8; doc_off [C+1] / tok: the view-m spans of the candidates alone"""
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    doc_off = doc_off - doc_off[0]
    tok = np.ascontiguousarray(tok, dtype=np.int32)
    assert len(tok) == doc_off[-1]
    off, flat, _ = flatten(items)
    out = np.zeros((len(off) - 1, len(doc_off) - 1), dtype=np.uint8)
    lib().xve_excluded(len(doc_off) - 1, ptr(doc_off), ptr(tok), len(off) - 1, ptr(off), ptr(flat), ptr(out))
    return out


def predict(S, n, ex=None, id0=0):
    """S [nq][C] -> (ids [nq][n] int64, scores [nq][n], counts [nq])"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    nq, Cn = S.shape
    ex = None if ex is None else np.ascontiguousarray(ex, dtype=np.uint8)
    assert ex is None or ex.shape == S.shape
    ids = np.zeros((nq, n), dtype=np.int64)
    sc = np.zeros((nq, n))
    counts = np.zeros(nq, dtype=np.int32)
    assert lib().xve_predict(nq, Cn, ptr(S), ptr(ex), int(n), int(id0), ptr(ids), ptr(sc), ptr(counts)) == 0
    return ids, sc, counts


def rank(S, query, cand, ex=None):
    """cand: column indices of S -> (score [P], rank [P] int64)"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    nq, Cn = S.shape
    ex = None if ex is None else np.ascontiguousarray(ex, dtype=np.uint8)
    query = np.ascontiguousarray(query, dtype=np.int64)
    cand = np.ascontiguousarray(cand, dtype=np.int64)
    assert query.shape == cand.shape and (len(query) == 0 or (query.min() >= 0 and query.max() < nq and cand.min() >= 0 and cand.max() < Cn))
    score = np.zeros(len(query))
    rk = np.zeros(len(query), dtype=np.int64)
    lib().xve_rank(Cn, ptr(S), ptr(ex), len(query), ptr(query), ptr(cand), ptr(score), ptr(rk))
    return score, rk


@dataclass
class Ranking:
    ids: np.ndarray
    scores: np.ndarray
    counts: np.ndarray
    stats: object = None
