"""ctypes wrapper of tests/native/emb_ref.c, the sequential restatement of TopicWordEmbeddings + TopicWordEmbeddingRunnable under the
device's draws and dot-product order (built once per process with gcc -O2 -ffp-contract=off into a temporary directory).  Test
infrastructure."""
import ctypes as C

import numpy as np

from tests.native_build import ptr, ref_lib

_lib = None


class ErTrain(C.Structure):
    _fields_ = [("doc_off", C.c_void_p), ("tok", C.c_void_p), ("z", C.c_void_p),
                ("D", C.c_int64), ("N0", C.c_int64), ("total_words", C.c_int64), ("ent_base", C.c_int64),
                ("V0", C.c_int32), ("C", C.c_int32), ("Cc", C.c_int32), ("window", C.c_int32), ("ns", C.c_int32),
                ("min_len", C.c_int32), ("epochs", C.c_int32), ("cache_size", C.c_int32),
                ("table_size", C.c_int64), ("table", C.c_void_p), ("retention", C.c_void_p), ("cache", C.c_void_p),
                ("min_exp", C.c_double), ("max_exp", C.c_double), ("seed", C.c_uint64), ("round", C.c_uint32), ("reserved", C.c_uint32)]


class ErStats(C.Structure):
    _fields_ = [("words", C.c_int64), ("sampled", C.c_int64), ("considered", C.c_int64), ("skipped", C.c_int64),
                ("calls", C.c_int64), ("negskip", C.c_int64), ("residual", C.c_double), ("last_residual", C.c_double),
                ("last_calls", C.c_int64)]


def lib():
    global _lib
    if _lib is None:
        L = ref_lib("emb_ref")
        vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
        L.er_philox.argtypes = [vp, vp, vp]
        L.er_draw64.argtypes = [u32, u32, u32, u32, u32, u32]; L.er_draw64.restype = u64
        L.er_cache.argtypes = [C.c_int, dbl, dbl, vp]
        L.er_init.argtypes = [i64, C.c_int, u64, vp, vp]
        L.er_count.argtypes = [C.c_int, i64, vp, dbl, vp, C.POINTER(i64), vp, vp, vp]
        L.er_table.argtypes = [C.c_int, vp, vp, i64, i64, i64, vp]
        L.er_table_literal.argtypes = [C.c_int, vp, vp, i64, vp]
        L.er_residual.argtypes = [dbl, dbl, C.c_int, vp, C.c_int, dbl, dbl]; L.er_residual.restype = dbl
        L.er_train.argtypes = [C.POINTER(ErTrain), vp, vp, C.POINTER(ErStats)]; L.er_train.restype = C.c_int
        L.er_softmax.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp]
        _lib = L
    return _lib


def philox(ctr, key):
    c = np.array(ctr, dtype=np.uint32); k = np.array(key, dtype=np.uint32); o = np.zeros(4, dtype=np.uint32)
    lib().er_philox(ptr(c), ptr(k), ptr(o))
    return [int(x) for x in o]


def cache(size=1000, min_exp=-6.0, max_exp=6.0):
    out = np.zeros(size + 1)
    lib().er_cache(size, min_exp, max_exp, ptr(out))
    return out


class EmbRef:
    """The state of one TopicWordEmbeddings (TWE:126-163) as the device keeps it; cfg: mvtopicmodel_amd.native.EmbConfig."""

    def __init__(self, V0, K, cfg, seed=0, weights=None):
        self.cfg, self.V0 = cfg, int(V0)
        self.K = int(K) if cfg.with_topics else 0
        self.Cc = int(cfg.num_context_columns) if cfg.with_topics else 0
        self.R, self.C = self.V0 + self.K, int(cfg.num_columns)
        self.w = np.zeros((self.R, self.C)); self.neg = np.zeros((self.R, self.C))
        if weights is None:
            lib().er_init(self.R, self.C, int(seed), ptr(self.w), ptr(self.neg))
        else:
            self.w[:] = weights
        self.cache = cache(cfg.sigmoid_cache_size, cfg.min_exp, cfg.max_exp)
        self.counts = np.zeros(self.V0, dtype=np.int64)
        self.total = 0
        self.sum_exp = np.zeros(self.K)

    def count_words(self, tok, table=True):
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        t = C.c_int64(self.total)
        self.retention = np.zeros(self.V0); self.sorted = np.zeros(self.V0, np.int32); self.dist = np.zeros(self.V0)
        lib().er_count(self.V0, len(tok), ptr(tok), float(self.cfg.sampling_factor), ptr(self.counts), C.byref(t),
                       ptr(self.retention), ptr(self.sorted), ptr(self.dist))
        self.total = t.value
        if table:
            self.table = self.table_range(0, self.cfg.sampling_table_size)

    def table_range(self, first, n):
        out = np.zeros(int(n), dtype=np.int32)
        lib().er_table(self.V0, ptr(self.sorted), ptr(self.dist), int(self.cfg.sampling_table_size), int(first), int(n), ptr(out))
        return out

    def table_at(self, idx):
        return np.array([self.table_range(int(i), 1)[0] for i in idx], dtype=np.int32)

    def table_literal(self):
        out = np.zeros(int(self.cfg.sampling_table_size), dtype=np.int32)
        lib().er_table_literal(self.V0, ptr(self.sorted), ptr(self.dist), int(self.cfg.sampling_table_size), ptr(out))
        return out

    def train(self, doc_off, tok, z, epochs, seed, round_idx=0, ent_base=0):
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64); tok = np.ascontiguousarray(tok, dtype=np.int32)
        z = None if (z is None or not self.K) else np.ascontiguousarray(z, dtype=np.int32)
        cfg = self.cfg
        a = ErTrain(ptr(doc_off), ptr(tok), ptr(z), len(doc_off) - 1, int(doc_off[-1]), int(self.total), int(ent_base),
                    self.V0, self.C, self.Cc, int(cfg.window), int(cfg.num_samples), int(cfg.min_doc_length), int(epochs),
                    int(cfg.sigmoid_cache_size), int(cfg.sampling_table_size), ptr(self.table), ptr(self.retention), ptr(self.cache),
                    float(cfg.min_exp), float(cfg.max_exp), int(seed), int(round_idx), 0)
        st = ErStats()
        assert lib().er_train(C.byref(a), ptr(self.w), ptr(self.neg), C.byref(st)) == 0
        return {f: getattr(st, f) for f, _ in ErStats._fields_}

    def softmax(self, reset_sums=False):
        if reset_sums:
            self.sum_exp[:] = 0.0
        e = np.zeros((self.K, self.V0))
        lib().er_softmax(self.V0, self.K, self.C, ptr(self.w), ptr(e), ptr(self.sum_exp))
        return e, self.sum_exp.copy()
