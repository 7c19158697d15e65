"""float64 numpy restatement of every step of csrc/kmeans.hip -- k-means++ seeding from given uniforms, the assignment with the lower-index
rule, the update with the empty-cluster rule, the fit, the two-proportion bin test with the Jensen-Shannon divergence, purity and normalised
mutual information -- from DIRECT differences (_prdc_ref.d2), not the Gram form the kernels use, with the input recipes of the tests and the
ambiguity condition a float32 Gram-form assignment is judged under."""
import functools
import math

import numpy as np

from _prdc_ref import d2, tol, case, lattice, U  # noqa: F401

MAX_K, MAX_CLASSES, ROW_BLOCK, NONFINITE, BAD_INDEX = 128, 32, 512, 1, 2
Z_5_PERCENT = 1.959963984540054


# ---- seeding -------------------------------------------------------------------------------------------------------------------------------
def pick(mind, u):
    """the first row whose running float64 sum of mind exceeds u * total; a total that is not positive: row floor(u n); no row above the
    target (rounding): the last row with a positive mind"""
    mind = np.asarray(mind, np.float64)
    n = len(mind)
    run = np.cumsum(mind)
    total = run[-1]
    if not total > 0.0:
        return min(int(math.floor(u * n)), n - 1)
    above = np.nonzero(run > u * total)[0]
    return int(above[0]) if len(above) else int(np.nonzero(mind > 0)[0][-1])


def seed(X, k, u):
    """-> (idx [k], the rows X[idx])"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    idx = [min(int(math.floor(u[0] * n)), n - 1)]
    mind = None
    for t in range(1, k):
        dist = np.maximum(d2(X, X[idx[-1]:idx[-1] + 1])[:, 0], 0.0)
        mind = dist if mind is None else np.minimum(mind, dist)
        idx.append(pick(mind, u[t]))
    idx = np.asarray(idx, np.int64)
    return idx, X[idx]


# ---- Lloyd ---------------------------------------------------------------------------------------------------------------------------------
def assign(X, C, D=None):
    """-> (the nearest centre, the LOWER index on a tie (np.argmin takes the first), that squared distance)"""
    D = d2(X, C) if D is None else D
    a = np.argmin(D, axis=1)
    return a, D[np.arange(D.shape[0]), a]


def update(X, a, C):
    """-> (centres: the mean of the members, an empty cluster keeps its centre; counts)"""
    X, C = np.asarray(X, np.float64), np.array(C, np.float64)
    counts = np.bincount(np.asarray(a)[(np.asarray(a) >= 0) & (np.asarray(a) < len(C))], minlength=len(C))
    for c in range(len(C)):
        if counts[c]:
            C[c] = X[np.asarray(a) == c].mean(axis=0)
    return C, counts


def fit(X, k, iters, u=None, idx=None):
    """seed (or the given seed rows idx), `iters` times (assign, update), a final assign -> dict(centres, idx, assign, counts, inertia
    [iters + 1], moved [iters + 1]; moved[0] = n)"""
    X = np.asarray(X, np.float64)
    if idx is None:
        idx, _ = seed(X, k, u)
    C = X[np.asarray(idx)].copy()
    inertia, moved, prev = [], [], None
    for t in range(iters + 1):
        a, dist = assign(X, C)
        inertia.append(float(np.sum(dist)))
        moved.append(len(a) if prev is None else int(np.sum(a != prev)))
        prev = a
        if t < iters:
            C, _ = update(X, a, C)
    return dict(centres=C, idx=np.asarray(idx), assign=prev, counts=np.bincount(prev, minlength=k), inertia=np.asarray(inertia),
                moved=np.asarray(moved))


# ---- the two scores (sums in the order the device takes: bins, clusters and classes ascending) ---------------------------------------------
def z_statistic(a, b, N1, N2):
    """(z, se) of one bin; se == 0: z is None"""
    p1, p2, P = a / N1, b / N2, (a + b) / (N1 + N2)
    se = math.sqrt(P * (1.0 - P) * (1.0 / N1 + 1.0 / N2))
    return (abs(p1 - p2) / se if se > 0.0 else None), se


def bin_test(ca, cb, z=Z_5_PERCENT):
    """-> (differing bins, their share, the Jensen-Shannon divergence in nats)"""
    ca, cb = [int(v) for v in ca], [int(v) for v in cb]
    N1, N2 = float(sum(ca)), float(sum(cb))
    nd, js = 0, 0.0
    for a, b in zip(ca, cb):
        a, b = float(a), float(b)
        stat, _ = z_statistic(a, b, N1, N2)
        nd += 1 if (stat is not None and stat > z) else 0
        p1, p2 = a / N1, b / N2
        m = 0.5 * (p1 + p2)
        t1 = p1 * math.log(p1 / m) if p1 > 0.0 else 0.0
        t2 = p2 * math.log(p2 / m) if p2 > 0.0 else 0.0
        js += 0.5 * t1 + 0.5 * t2
    return nd, nd / float(len(ca)), js


def contingency(a, y, k, classes):
    table = np.zeros((k, classes), np.int64)
    np.add.at(table, (np.asarray(a), np.asarray(y)), 1)
    return table


def cluster_scores(a, y, k, classes):
    """-> (purity, NMI = I / ((H(U) + H(V)) / 2), 1 when both entropies are 0, the contingency table [k, classes])"""
    table = contingency(a, y, k, classes)
    n = float(len(a))
    rows, cols = table.sum(axis=1), table.sum(axis=0)
    mi = 0.0
    for c in range(k):
        s = 0.0
        for j in range(classes):
            v = int(table[c, j])
            if v > 0:
                s += (v / n) * math.log((v * n) / (float(rows[c]) * float(cols[j])))
        mi += s
    hu = -sum((r / n) * math.log(r / n) for r in rows.tolist() if r > 0)
    hv = -sum((r / n) * math.log(r / n) for r in cols.tolist() if r > 0)
    purity = float(table.max(axis=1).sum()) / n
    nmi = 1.0 if (hu == 0.0 and hv == 0.0) else mi / (0.5 * (hu + hv))
    return purity, nmi, table


# ---- the assignment cases: rows of _prdc_ref.case, centres k of them by a seeded permutation, and the same after 3 float64 Lloyd iterations
ASSIGN_CASES = [(1, 10), (3, 37), (16, 100), (127, 37), (128, 100), (784, 100), (3072, 37)]
AMBIGUOUS_CAP = 0.05            # the share of rows of a case that may be ambiguous: a condition on the cases, asserted for the restatement
                                # alone by the CPU test (it stays at 2.7 % or below there)


def assign_rows(d):
    return case(1000, 67, d)[0][:600 if d == 3072 else 1000]


@functools.lru_cache(maxsize=None)
def assign_case(d, k, lloyd):
    """(X float32 [rows, d], C float32 [k, d], D float64 [rows, k] of the two, T float64 [rows]: the row's float32 Gram tolerance), made once
    per run and never written to"""
    X = assign_rows(d)
    rng = np.random.RandomState(d + k)
    C = np.asarray(X, np.float64)[rng.permutation(X.shape[0])[:k]].copy()
    for _ in range(lloyd):
        C, _ = update(X, assign(X, C)[0], C)
    C = C.astype(np.float32)
    D, T = d2(X, C), tol(X, C).max(axis=1)
    for arr in (C, D, T):
        arr.setflags(write=False)
    return X, C, D, T


def ambiguous(D, T):
    """rows whose second smallest distance is within 2 T of the smallest: either centre may win in float32"""
    s = np.sort(D, axis=1)
    if D.shape[1] < 2:
        return np.zeros(D.shape[0], bool)
    return (s[:, 1] - s[:, 0]) <= 2.0 * T
