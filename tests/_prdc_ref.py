"""float64 restatement of the k-NN-ball scores (improved precision / recall, Kynkaanniemi et al. 2019; density / coverage, Naeem et al.
2020) from DIRECT differences -- not the Gram form the kernels use --, the input recipe of the tests, and the tolerance a float32
Gram-form distance is allowed.  Squared Euclidean distances throughout; comparisons inclusive; self left out by index."""
import functools

import numpy as np

U = 2.0 ** -23          # the unit roundoff the bound is stated with


def d2(A, B):
    """[m, n] squared distances from direct differences in float64 (row by row: nothing of size m n d is held)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        diff = B - A[i]
        out[i] = np.einsum('jk,jk->j', diff, diff)
    return out


def radii_from(D, k):
    """D: the [n, n] distances of a set to itself -> the k-th smallest of each row without its own index (a multiset order statistic)"""
    n = D.shape[0]
    assert 1 <= k <= n - 1
    off = D[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.sort(off, axis=1)[:, k - 1]


def radii(Z, k):
    return radii_from(d2(Z, Z), k)


def ball_counts(A, B, rB):
    """per row a of A: (#{j: |a - b_j|^2 <= rB[j]}, min_j |a - b_j|^2)"""
    D = d2(A, B)
    return (D <= np.asarray(rB, np.float64)[None, :]).sum(1), D.min(1)


def scores(cnt_y, cnt_x, mn_x, r_x, k):
    """(precision, recall, density, coverage) from ball_counts(Y, X, r_X) and ball_counts(X, Y, r_Y)"""
    n, m = len(cnt_y), len(cnt_x)
    return (float(np.mean(cnt_y > 0)), float(np.mean(cnt_x > 0)), float(np.sum(cnt_y)) / (k * n), float(np.mean(mn_x <= r_x)))


def prdc(X, Y, k):
    r_x, r_y = radii(X, k), radii(Y, k)
    cnt_y, _ = ball_counts(Y, X, r_x)
    cnt_x, mn_x = ball_counts(X, Y, r_y)
    return scores(cnt_y, cnt_x, mn_x, r_x, k)


# ---- the tolerance (derived): a float32 Gram-form distance n_i + n_j - 2 g_ij with float32 norms, accumulated in any order, is off from the
# exact one by at most T_ij = (2 d + 4) u (|a_i|^2 + |b_j|^2) -- d products and d - 1 additions per dot product, three of them, and the
# three-term combination
def tol(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return (2 * A.shape[1] + 4) * U * ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :])


def count_brackets(D, rB, T):
    """(lo, hi, mn) per row of D [m, n]: the counts no / every pair within T of its threshold belongs to"""
    rB = np.asarray(rB, np.float64)[None, :]
    return (D <= rB - T).sum(1), (D <= rB + T).sum(1), D.min(1)


def score_brackets(X, Y, k, doubled=True, D=None):
    """what a float32 Gram-form computation of prdc(X, Y, k) may return: dict(lo=(P, R, D, C), hi=(P, R, D, C), ambiguous=share of rows
    whose count bracket is open, rows=(lo_y, hi_y, lo_x, hi_x)).  doubled: the radii are the op's own (end to end: 2 T + u max r); else
    float32 casts of the reference's (T + u r).  D: (d2(X, X), d2(Y, Y), d2(X, Y)) where the caller has them."""
    Dxx, Dyy, Dxy = D if D is not None else (d2(X, X), d2(Y, Y), d2(X, Y))
    r_x, r_y = radii_from(Dxx, k), radii_from(Dyy, k)
    Txy = tol(X, Y)
    if doubled:
        Ty, Tx = 2 * Txy.T + U * r_x.max(), 2 * Txy + U * r_y.max()
    else:
        Ty, Tx = Txy.T + U * r_x[None, :], Txy + U * r_y[None, :]
    lo_y, hi_y, _ = count_brackets(Dxy.T, r_x, Ty)             # generated rows in real balls
    lo_x, hi_x, mn_x = count_brackets(Dxy, r_y, Tx)            # real rows in generated balls
    tc = Tx.max(1)                                             # coverage: mn <= r_x within the row's tolerance
    lo = scores(lo_y, lo_x, mn_x + tc, r_x, k)
    hi = scores(hi_y, hi_x, mn_x - tc, r_x, k)
    amb = (np.sum(lo_y != hi_y) + np.sum(lo_x != hi_x)) / float(len(lo_y) + len(lo_x))
    return dict(lo=lo, hi=hi, ambiguous=float(amb), rows=(lo_y, hi_y, lo_x, hi_x), r_x=r_x, r_y=r_y, mn_x=mn_x, tc=tc)


# ---- inputs: low-dimensional modes in d dimensions, a generated set that misses one mode and has a fifth of its rows off the manifold
CASES = [(130, 67, 33), (257, 300, 131), (192, 160, 3072), (5, 9, 16)]
KNOWN = {((130, 67, 33), 3): (.761, .662, .940, .546), ((257, 300, 131), 5): (.837, .747, .849, .743),
         ((192, 160, 3072), 3): (.719, .693, .744, .578), ((5, 9, 16), 1): (.333, .800, .444, .600)}


@functools.lru_cache(maxsize=None)
def case(m, n, d):
    """(X [m, d], Y [n, d]) float32, read-only, made once per run"""
    rng = np.random.default_rng(1000 * m + 10 * n + d)
    q = min(4, d)
    cen = rng.standard_normal((4, d))
    bas = rng.standard_normal((4, q, d)) / np.sqrt(q)

    def draw(rows, modes):
        c = rng.integers(0, modes, size=rows)
        t = rng.standard_normal((rows, q))
        return cen[c] + np.einsum('iq,iqd->id', t, bas[c]) + 0.05 * rng.standard_normal((rows, d))
    X = draw(m, 4)
    Y = draw(n, 3)
    Y[:n // 5] += 0.8 * rng.standard_normal((n // 5, d))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def case_d2(m, n, d):
    """(d2(X, X), d2(Y, Y), d2(X, Y)) of case(m, n, d), computed once per run and never written to"""
    X, Y = case(m, n, d)
    D = (d2(X, X), d2(Y, Y), d2(X, Y))
    for a in D:
        a.setflags(write=False)
    return D


def lattice(m, n, d):
    """integer entries in {0, 1, 2, 3}: every product and sum of the Gram form is exact in float32"""
    rng = np.random.default_rng(7 * m + n + d)
    return rng.integers(0, 4, size=(m, d)).astype(np.float32), rng.integers(0, 4, size=(n, d)).astype(np.float32)
