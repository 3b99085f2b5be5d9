"""ctypes wrapper of tests/native/gram_ref.c, the sequential restatement of the topic-map contract of include/mvhdp.h (mvhdp_topic_gram):
built once per process with gcc -O2 -ffp-contract=off into a temporary directory.  phi and theta are not restated here: phi is
xview_ref.phi_table, theta is what mvhdp_doc_topic_proportions returns for the handle under test.  Test infrastructure: no GPU, no product
code."""
import ctypes as C

import numpy as np

from tests.native_build import ptr, ref_lib

BLOCK_ROWS = 1024
CONTRACT, DESCENDING, UNFUSED, OTHER_BLOCK, ONE_CHAIN = 0, 1, 2, 3, 4     # gram_ref's variants: the contract, and four the sensitivity tests run
TRANSFORMS = {"identity": 0, "sqrt": 1}
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("gram_ref")
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.gram_ref.argtypes = [i32, i64, vp, i32, i32, i64, vp, vp]
        L.gram_ref.restype = i32
        L.gram_counts.argtypes = [i32, i64, vp, dbl, vp, vp]
        L.gram_counts.restype = None
        _lib = L
    return _lib


def gram(x, transform="identity", variant=CONTRACT, block=BLOCK_ROWS):
    """(gram [K][K], sums [K]) of the rows x [n][K]"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, K = x.shape
    g, s = np.zeros((K, K)), np.zeros(K)
    src = x if n else np.zeros((1, K))
    assert lib().gram_ref(K, n, ptr(src), TRANSFORMS[transform], int(variant), int(block), ptr(g), ptr(s)) == 0
    return g, s


def counts(x, threshold):
    """(n_above [K], co_above [K][K]) of the rows x [n][K]"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, K = x.shape
    na, co = np.zeros(K, dtype=np.int64), np.zeros((K, K), dtype=np.int64)
    src = x if n else np.zeros((1, K))
    lib().gram_counts(K, n, ptr(src), float(threshold), ptr(na), ptr(co))
    return na, co


def topic_gram(x, transform="identity", threshold=None):
    """the restatement as a TopicGram (the product's dataclass: a container, no device)"""
    from mvtopicmodel_amd.native import TopicGram
    g, s = gram(x, transform)
    na, co = counts(x, threshold) if threshold is not None else (None, None)
    return TopicGram(g, s, na, co, len(x), transform)
