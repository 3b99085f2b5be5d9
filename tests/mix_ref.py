"""ctypes wrapper of tests/native/mix_ref.c: the deferred sweep with the useVectorsLambda mix of view 0, restated sequentially on the
CPU oracle's model object and primitives (built once per process with gcc -O2 -ffp-contract=off into a temporary directory and linked
against the oracle's library).  Test infrastructure.

MixRef is an Oracle whose build_trees / sweep / sweep_list know the mix: set_vectors_mix(lam, e, S) with the reference's tables
expDotProductValues [K][V_0] / sumExpValues [K].  lam = 0 switches the mix off (the oracle's arithmetic); through_mix_path=True keeps
the table and runs lam = 0 through the mix expression (0 + 1 * q), which must give the same bits."""
import ctypes as C
import os

import numpy as np

from oracle import binding as ob
from oracle.binding import Oracle, Stats, _ptr
from tests.native_build import ref_lib

_lib = None
TRACE_PRODUCT = 0x100                                    # MXR_TRACE_PRODUCT


def lib():
    global _lib
    if _lib is None:
        ob.lib()                                        # (builds the oracle's library when it is missing or stale)
        odir = os.path.dirname(ob._SO)
        L = ref_lib("mix_ref", extra_flags=("-fno-fast-math", "-Wall"), link=("-L" + odir, "-lmvhdp_oracle", "-Wl,-rpath," + odir, "-lm"))
        vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
        L.mxr_make_mix.argtypes = [C.c_int, C.c_int, dbl, vp, vp, vp]
        L.mxr_build_trees.argtypes = [vp, C.c_int, vp, dbl]
        L.mxr_sweep.argtypes = [vp, C.c_int, vp, dbl, u32, u64, i64, vp, u32, C.POINTER(Stats), vp, vp, vp,
                                C.c_int, vp, vp, vp, vp, vp, i64]
        L.mxr_sweep.restype = C.c_int
        _lib = L
    return _lib


def make_mix(lam, exp_dot, sum_exp):
    """lam * (e[k][w] / S[k]) as [V_0][K]: what mvhdp_get_vectors_mix returns."""
    e = np.ascontiguousarray(exp_dot, dtype=np.float64)
    s = np.ascontiguousarray(sum_exp, dtype=np.float64)
    K, V0 = e.shape
    assert s.shape == (K,)
    out = np.empty((V0, K), dtype=np.float64)
    lib().mxr_make_mix(V0, K, float(lam), _ptr(e), _ptr(s), _ptr(out))
    return out


class MixRef(Oracle):
    def __init__(self, K, V):
        super().__init__(K, V)
        self.X = lib()
        self.lam = 0.0
        self.mix = None                                  # [V_0][K] or None: off
        self.oml = 1.0

    def set_vectors_mix(self, lam, exp_dot=None, sum_exp=None, through_mix_path=False):
        lam = float(lam)
        assert 0.0 <= lam <= 1.0
        if lam == 0.0 and not through_mix_path:
            self.lam, self.mix, self.oml = 0.0, None, 1.0
            return
        self.lam = lam
        self.mix = make_mix(lam, exp_dot, sum_exp)
        assert self.mix.shape == (self.V[0], self.K)
        self.oml = 1.0 - lam

    def build_trees(self):
        self.X.mxr_build_trees(self.h, 0 if self.mix is None else 1, _ptr(self.mix), self.oml)

    def _sweep(self, sweep_idx, seed, p, flags, doc_id_base, want_delta, want_dbg, trace, docs):
        st = Stats()
        dn = np.zeros((sum(self.V), self.K), dtype=np.int32) if want_delta else None
        dk = np.zeros((self.M, self.K), dtype=np.int32) if want_delta else None
        dbg = dbg_ptrs = None
        if want_dbg:
            dbg = [np.zeros((max(self.N[m], 1), 4), dtype=np.float64) for m in range(self.M)]
            dbg_ptrs = (C.c_void_p * self.M)(*[d.ctypes.data for d in dbg])
        if p is not None:
            p = np.ascontiguousarray(p, dtype=np.float64)
            assert p.shape == (self.D, self.M, self.M)
        nt, td, tv, tp, tout = 0, None, None, None, None
        if trace is not None and len(trace) > 0:
            nt = len(trace)
            td = np.ascontiguousarray([t[0] for t in trace], dtype=np.int64)
            tv = np.ascontiguousarray([t[1] for t in trace], dtype=np.int32)
            tp = np.ascontiguousarray([t[2] for t in trace], dtype=np.int32)
            tout = np.zeros((nt, self.K + 1), dtype=np.float64)
        dl = keep = None
        if docs is not None:                             # (an empty list is still a list: a non-null pointer)
            docs = np.ascontiguousarray(docs, dtype=np.int64)
            keep = docs if len(docs) else np.zeros(1, dtype=np.int64)
            dl = _ptr(keep)
        rc = self.X.mxr_sweep(self.h, 0 if self.mix is None else 1, _ptr(self.mix), self.oml, int(sweep_idx), int(seed), int(doc_id_base),
                              _ptr(p), int(flags), C.byref(st), _ptr(dn), _ptr(dk),
                              C.cast(dbg_ptrs, C.c_void_p) if dbg_ptrs is not None else None,
                              nt, _ptr(td), _ptr(tv), _ptr(tp), _ptr(tout), dl, 0 if docs is None else len(docs))
        if rc:
            raise RuntimeError(f"mxr_sweep rc={rc}")
        return dict(stats=st.as_dict(), delta_nwk=dn, delta_nk=dk,
                    dbg=[d[: self.N[m]] for m, d in enumerate(dbg)] if dbg else None, trace=tout)

    def sweep(self, sweep_idx, seed, p=None, flags=0, doc_id_base=0, want_delta=False, want_dbg=False, trace=None, trace_product=False):
        """trace_product: a listed topic's traced share from the product (p_mm n + other) p_wt, as the register-resident kernels form it,
        instead of the difference of two running sums (the oracle's form, and the generic kernel's)"""
        return self._sweep(sweep_idx, seed, p, flags | (TRACE_PRODUCT if trace_product else 0), doc_id_base, want_delta, want_dbg, trace, None)

    def sweep_list(self, sweep_idx, seed, docs, p=None, flags=0, doc_id_base=0, want_delta=False):
        return self._sweep(sweep_idx, seed, p, flags, doc_id_base, want_delta, False, None, docs)
