"""Inputs of the topic-map tests (mvhdp_topic_gram), made on the host alone: host rows of every shape at which the device code takes
another path, rows with special values, and the multi-view corpora of tests/xview_cases.py sized so that entities and types span several
blocks of 1024 rows.  Test infrastructure."""
import numpy as np

from tests import xview_cases as xc

# the tile is 64 (k) x 128 (l) cells, the co-occurrence tile 64 x 64, the mask tile 64 topics
K_VALUES = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200]
# the slab is 16 rows, a mask word 64 rows, a block 1024 rows (= the 16 mask words staged at once)
ROW_VALUES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2048, 3 * 1024 + 5]
BLOCKS_PER_PASS = [0, 1, 2]                      # 3 * 1024 + 5 rows are four blocks: four passes, two passes
THRESHOLD = 0.5


def rows(n, K, seed=0):
    """[n][K] in [0, 1): a third of the entries exactly 0.0, a few exactly at THRESHOLD and one ulp above it"""
    rng = np.random.default_rng(10007 * K + n + seed)
    x = rng.random((n, K))
    x[rng.random((n, K)) < 1 / 3] = 0.0
    at = rng.random((n, K))
    x[at < 0.02] = THRESHOLD
    x[(at >= 0.02) & (at < 0.04)] = np.nextafter(THRESHOLD, 1.0)
    return x


def wide_rows(n, K, seed=0):
    """[n][K] with magnitudes from 2^-300 to 2^300, for the sqrt transform"""
    rng = np.random.default_rng(31 * K + n + seed)
    return np.ldexp(1.0 + rng.random((n, K)), rng.integers(-300, 300, (n, K)))


def model(K, Vm, D, seed=0, inactive=None):
    """a three-view corpus: view 1 has Vm types, a tenth of the entities lack any given view"""
    return xc.make(K, Vm, D, 3, seed=seed, inactive=inactive)


def lacks_a_weighted_view(c, weights):
    """[D] bool: the entity has no tokens in a view whose weight is not 0 -- its proportions carry the earlier entity's counts over"""
    out = np.zeros(c.D, dtype=bool)
    for v in range(c.M):
        if weights[v] > 0:
            out |= np.diff(c.doc_off[v]) == 0
    return out
