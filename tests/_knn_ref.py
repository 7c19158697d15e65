"""float64 restatement of the labelled neighbour lists (ggan_knn_lists / ggan_knn_vote, functional.knn_lists / knn_vote / knn_accuracy) from
DIRECT differences -- not the Gram form the kernel uses --, the labelled input recipe of the tests, and the rule that says which rows a
float32 Gram-form computation is allowed to decide differently.  Distances, their tolerance and the integer lattice are _prdc_ref's.

Lists are ascending in the total order (distance, candidate index); a vote goes to the most frequent label, the smallest one on a tie;
leave-one-out leaves candidate i out for query i by index.

Which rows float32 may decide differently (derived, not measured): a float32 Gram-form distance of row i is within T_i = max_j tol(Q, C)[i, j]
of the exact one.  With d_k the reference's k-th distance of row i, a candidate with D < d_k - 2 T_i is nearer than the k-th in float32
too (each of the two moves by at most T_i), so it is in every float32 list, and one with D > d_k + 2 T_i is in none.  The candidates of
the band [d_k - 2 T_i, d_k + 2 T_i] are the ones float32 may swap.
  set-closed    the band holds the k-th neighbour alone: the float32 list equals the reference's as a set, and position for position
                wherever the reference's consecutive distances differ by more than 2 T_i on both sides;
  label-closed  every candidate of the band carries one label: whichever of them float32 picks, the label multiset is the reference's, so
                the vote is the reference's exactly."""
import functools

import numpy as np

from _prdc_ref import U, d2, lattice, tol  # noqa: F401

CLASSES = 4


def distances(Q, C, skip_diag=False):
    """[m, n] float64 squared distances; leave-one-out: the diagonal is +inf (candidate i does not exist for query i)"""
    D = d2(Q, C)
    if skip_diag:
        assert D.shape[0] == D.shape[1]
        D = D.copy()
        D[np.arange(D.shape[0]), np.arange(D.shape[0])] = np.inf
    return D


def lists_from(D, k):
    """(idx [m, k] int64, dist [m, k]): per row the k smallest under (distance, index), by np.lexsort((index, D))"""
    m, n = D.shape
    assert 1 <= k <= n
    J = np.broadcast_to(np.arange(n), (m, n))
    order = np.lexsort((J, D), axis=-1)[:, :k]
    return order, np.take_along_axis(D, order, axis=1)


def lists(Q, C, k, skip_diag=False):
    return lists_from(distances(Q, C, skip_diag), k)


def vote(idx, labels_c):
    """pred [m]: np.argmax(np.bincount(labels of the list)) -- the smallest label wins a tie"""
    labels_c = np.asarray(labels_c, np.int64)
    return np.array([int(np.argmax(np.bincount(labels_c[row]))) for row in np.asarray(idx)], np.int64)


def confusion(labels_q, pred, classes):
    out = np.zeros((classes, classes), np.int64)
    np.add.at(out, (np.asarray(labels_q, np.int64), np.asarray(pred, np.int64)), 1)
    return out


def accuracy(Z, y, k):
    """leave-one-out k-NN accuracy in float64"""
    idx, _ = lists(Z, Z, k, skip_diag=True)
    return float(np.mean(vote(idx, y) == np.asarray(y)))


def row_tol(Q, C):
    """T_i = max_j tol(Q, C)[i, j]"""
    return tol(Q, C).max(1)


def closed_rows(D, k, T, labels_c=None):
    """what float32 may not decide differently, from the reference alone.  D [m, n] (diagonal +inf for leave-one-out), T [m] ->
    dict(idx, dist: the reference's lists; set_closed [m]; pinned [m, k]: positions of set-closed rows that must match as a sequence;
    label_closed [m] (with labels_c))"""
    idx, dist = lists_from(D, k)
    dk, T2 = dist[:, -1:], 2.0 * np.asarray(T)[:, None]
    band = (D >= dk - T2) & (D <= dk + T2)
    set_closed = band.sum(1) == 1
    gap = np.diff(dist, axis=1) > T2                                  # [m, k - 1]: position q + 1 is clear of position q
    below = np.concatenate([np.ones((len(D), 1), bool), gap], axis=1)
    above = np.concatenate([gap, np.ones((len(D), 1), bool)], axis=1)   # (the k-th is clear of the k+1-th in a set-closed row)
    out = dict(idx=idx, dist=dist, set_closed=set_closed, pinned=below & above & set_closed[:, None])
    if labels_c is not None:
        lab = np.broadcast_to(np.asarray(labels_c, np.int64), D.shape)
        lo = np.where(band, lab, np.iinfo(np.int64).max).min(1)
        hi = np.where(band, lab, np.iinfo(np.int64).min).max(1)
        out['label_closed'] = lo == hi
    return out


def accuracy_bracket(pred_ref, labels_q, label_closed):
    """(lo, hi): every label-closed row counts as the reference says, an open row may go either way"""
    ok = (np.asarray(pred_ref) == np.asarray(labels_q)) & label_closed
    lo = float(np.mean(ok))
    return lo, lo + float(np.mean(~label_closed))


@functools.lru_cache(maxsize=None)
def labelled(n, d):
    """(Z [n, d] float32, y [n] int32), read-only, made once per run: four classes, each a 4-dimensional Gaussian sheet around its
    centre, isotropic noise on top; a fifth of the labels redrawn uniformly, so that the accuracy is neither 0 nor 1.
    Draw order: centres, bases, classes, sheet coordinates, noise (generator 31 n + d); redrawn rows, their labels (generator 5 n + d)."""
    rng = np.random.default_rng(31 * n + d)
    cen = 1.5 * rng.standard_normal((CLASSES, d)) / np.sqrt(d)
    bas = rng.standard_normal((CLASSES, 4, d)) / np.sqrt(d)
    y = rng.integers(0, CLASSES, size=n)
    t = rng.standard_normal((n, 4))
    Z = cen[y] + np.einsum('iq,iqd->id', t, bas[y]) + 0.3 * rng.standard_normal((n, d)) / np.sqrt(d)
    rng2 = np.random.default_rng(5 * n + d)
    redrawn = rng2.permutation(n)[:n // 5]
    y[redrawn] = rng2.integers(0, CLASSES, size=len(redrawn))
    Z, y = Z.astype(np.float32), y.astype(np.int32)
    Z.setflags(write=False)
    y.setflags(write=False)
    return Z, y


def split(m, n, d):
    """queries and bank out of ONE labelled set of m + n rows: (Q [m, d], yq, C [n, d], yc)"""
    Z, y = labelled(m + n, d)
    return Z[:m], y[:m], Z[m:], y[m:]


@functools.lru_cache(maxsize=None)
def reference(m, n, d, k, skip_diag):
    """closed_rows (+ T, pred, D) of the shared float cases, computed once per run and never written to: skip_diag -> labelled(n, d)
    against itself, else split(m, n, d)"""
    if skip_diag:
        assert m == n
        C, yc = labelled(n, d)
        Q, yq = C, yc
    else:
        Q, yq, C, yc = split(m, n, d)
    D, T = distances(Q, C, skip_diag), row_tol(Q, C)
    out = closed_rows(D, k, T, yc)
    out.update(D=D, T=T, pred=vote(out['idx'], yc), Q=Q, C=C, yq=yq, yc=yc)
    return out
