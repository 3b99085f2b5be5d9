"""Inputs of the cross-view prediction tests, made on the host alone: a small multi-view corpus with assignments, its counts, the
hyper-parameters, and a host evaluation of the topic proportions.  tests/test_gpu_xview.py loads exactly these into a sampler;
tests/test_xview_kats.py measures on them how far a reordered or unfused chain moves the scores.  Test infrastructure."""
from dataclasses import dataclass

import numpy as np

from mvtopicmodel_amd.native import Hyper

# (K, V of the predicted view, D, M): every K of {1, 5, 64, 100, 257, 400}, every V_m of {1, 3, 127, 128, 129, 1000}, every D of
# {1, 65, 300} at least once; M = 3 predicts view 1 from views 0 and 2, M = 1 predicts the view from itself
SHAPES = [(1, 1, 1, 1), (5, 3, 65, 3), (64, 127, 300, 3), (100, 128, 65, 3), (257, 129, 300, 1), (400, 1000, 65, 3), (64, 1000, 65, 1), (5, 129, 1, 3)]


@dataclass
class Case:
    K: int
    V: list
    D: int
    M: int
    m: int                     # the predicted view
    weights: np.ndarray        # [M] view weights: 0 for the predicted view when there are others
    doc_off: list              # per view [D + 1]
    tokens: list
    z: list
    hy: Hyper
    full: int                  # the entity whose view-m span holds every type (-1: none)
    no_target: int             # an entity without view m (-1: none)
    no_source: int             # an entity without any other view (-1: none)

    def counts(self, v):
        nwk = np.zeros((self.V[v], self.K), dtype=np.int32)
        np.add.at(nwk, (self.tokens[v], self.z[v]), 1)
        return nwk, nwk.sum(0).astype(np.int32)

    def theta(self):
        """[D][K]: the formula of mvhdp_doc_topic_proportions with its carry-over, in numpy (the bits of the device are not claimed)"""
        K, hy = self.K, self.hy
        out = np.zeros((self.D, K))
        for v in range(self.M):
            ndk, length = np.zeros(K), 0
            for d in range(self.D):
                b, e = self.doc_off[v][d], self.doc_off[v][d + 1]
                if e > b:
                    ndk, length = np.bincount(self.z[v][b:e], minlength=K).astype(np.float64), e - b
                out[d] += self.weights[v] * (ndk + hy.gamma[v] * hy.alpha[v, :K]) / (length + hy.gamma[v] * hy.alpha_sum[v])
        return out / self.weights.sum()


def make(K, Vm, D, M, seed=0, inactive=None):
    rng = np.random.default_rng(1000 * K + Vm + D + seed)
    m = 1 if M == 3 else 0
    V = [60, Vm, 25] if M == 3 else [Vm]
    mean_len = [30, 6, 8] if M == 3 else [12]
    full = 1 if D > 1 else -1
    no_target = 3 if D > 4 else -1
    no_source = 5 if D > 6 and M > 1 else -1
    active = np.flatnonzero(~np.asarray(inactive, dtype=bool)) if inactive is not None else np.arange(K)
    doc_off, tokens, zs = [], [], []
    for v in range(M):
        lens = rng.integers(0, 2 * mean_len[v], D)
        lens[rng.random(D) < 0.1] = 0                                        # entities without the view, here and there
        if D == 1:
            lens[0] = max(int(lens[0]), 2)
        if v == m:
            if no_target >= 0:
                lens[no_target] = 0
            if no_source >= 0:
                lens[no_source] = 4
            if full >= 0:
                lens[full] = V[v]
        elif no_source >= 0:
            lens[no_source] = 0
            lens[no_source - 1] = max(int(lens[no_source - 1]), 3)           # the entity it carries over from has the view
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        top = max(1, V[v] - 2) if v == m else V[v]                           # the last two types of view m occur in `full` alone
        tok = rng.integers(0, top, off[-1]).astype(np.int32)
        z = active[(tok.astype(np.int64) * 7 + rng.integers(0, 3, len(tok))) % len(active)].astype(np.int32)   # sparse rows: three topics a type
        if v == m and full >= 0:
            tok[off[full]:off[full + 1]] = np.arange(V[v], dtype=np.int32)
            z[off[full + 1] - min(2, V[v]):off[full + 1]] = z[off[full + 1] - 1]         # ... once each, under one topic: two equal count rows
        doc_off.append(off); tokens.append(tok); zs.append(z)
    hy = Hyper.defaults(K, V, inactive=inactive)
    hy.alpha[:, :K] = rng.uniform(0.05, 0.15, (M, K))
    hy.alpha_sum = hy.alpha[:, :K].sum(1) * 1.25
    hy.gamma = np.linspace(0.8, 0.9, M)
    weights = np.array([1.0, 0.0, 0.7]) if M == 3 else np.array([1.0])
    return Case(K, V, D, M, m, weights, doc_off, tokens, zs, hy, full, no_target, no_source)
