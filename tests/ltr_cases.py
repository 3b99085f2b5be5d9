"""Cases shared by the CPU and the GPU tests of the left-to-right held-out estimator: the two-token document whose second position has an
exactly enumerable expectation, and the synthetic held-out documents with out-of-vocabulary tokens at chosen places."""
import math

import numpy as np

# ---- L = 2, K = 3: position 1 is exactly unbiased for p(w_1 | w_0) -------------------------------------------------------------------
PEAKED_NWK = np.array([[90, 5, 5], [2, 3, 95]], dtype=np.int32)             # word 0 lives in topic 0, word 1 in topic 2
PEAKED_NK = PEAKED_NWK.sum(0).astype(np.int32)
PEAKED_BETA = 0.01
PEAKED_ALPHA = np.array([0.05, 0.05, 0.05])
PEAKED_ALPHA_SUM = 0.15
PEAKED_R = 4096
PEAKED_DOC = (np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32))


def peaked_expectation():
    """(exact p(w_1 | w_0), a, b, Hoeffding half-width at R = PEAKED_R and failure probability 1e-9, the two values a version that forgets
    the earlier token would return), all enumerated here"""
    V, K = PEAKED_NWK.shape
    phi = (PEAKED_NWK + PEAKED_BETA) / (PEAKED_NK + PEAKED_BETA * V)         # [w][k]
    post = PEAKED_ALPHA * phi[0]
    post = post / post.sum()                                                 # P(z_0 | w_0)
    given = np.array([((PEAKED_ALPHA + (np.arange(K) == z0)) * phi[1]).sum() / (PEAKED_ALPHA_SUM + 1) for z0 in range(K)])
    exact = float((post * given).sum())
    a, b = float(given.min()), float(given.max())
    half = (b - a) * math.sqrt(math.log(2 / 1e-9) / (2 * PEAKED_R))
    forgets = [float((PEAKED_ALPHA * phi[1]).sum() / PEAKED_ALPHA_SUM), float((PEAKED_ALPHA * phi[1]).sum() / (PEAKED_ALPHA_SUM + 1))]
    return exact, a, b, half, forgets


# ---- held-out documents: the lengths at which the kernel changes its path, out-of-vocabulary tokens first, in the middle, last ----------
LENGTHS = [0, 1, 2, 63, 64, 65, 130]


def heldout_docs(V, n_docs=40, seed=1, lengths=LENGTHS):
    """n_docs documents with lengths drawn from `lengths` (each at least once), tokens uniform over [0, V); every second document of length
    >= 2 gets an out-of-vocabulary token (V, V + 7 or 2^31 - 1) at its first, a middle or its last position, and one document of length 2 is
    out of vocabulary throughout"""
    rng = np.random.default_rng(seed)
    lens = np.array(list(lengths) + list(rng.choice(lengths, n_docs - len(lengths))))
    rng.shuffle(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = rng.integers(0, V, off[-1]).astype(np.int32)
    oov = [V, V + 7, 2 ** 31 - 1]
    marked = 0
    for i, d in enumerate(d for d in range(n_docs) if lens[d] >= 2):
        if i % 2 == 0:
            L = int(lens[d])
            where = [0, L // 2, L - 1][marked % 3]
            tok[off[d] + where] = oov[marked % 3]
            marked += 1
    twos = [d for d in range(n_docs) if lens[d] == 2]
    tok[off[twos[-1]]:off[twos[-1] + 1]] = V
    assert marked >= 3
    return off, tok


# ---- the header's summation order, written once more in Python (for known answers that are equalities) -------------------------------
def lane_order_total(wt):
    """sum of the K weights in the order include/mvhdp.h fixes: lane l adds its T topics in ascending order, the 64 lane sums are scanned
    (four in-row steps, lanes 16..31 and 48..63 add lanes 15 and 47, lanes 32..63 add lane 31); the total is lane 63's value"""
    K = len(wt)
    T = 1
    while 64 * T < K:
        T *= 2
    w = [float(x) for x in wt] + [0.0] * (64 * T - K)
    v = []
    for l in range(64):
        run = w[l * T]
        for j in range(1, T):
            run = run + w[l * T + j]
        v.append(run)
    for s in (1, 2, 4, 8):
        v = [v[l] + v[l - s] if (l & 15) >= s else v[l] for l in range(64)]
    v = [v[l] + v[15] if 16 <= l < 32 else v[l] + v[47] if l >= 48 else v[l] for l in range(64)]
    v = [v[l] + v[31] if l >= 32 else v[l] for l in range(64)]
    return v[63]
