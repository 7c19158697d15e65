"""k-means fitted on the device and the two scores read off a fitted partition (csrc/kmeans.hip): thin wrappers, forward only, device
tensors in and out, nothing is read back."""
import collections

import numpy as np

from ._core import torch, _lib, check, _L, _p, _stream, _c, _dev
from .rows import _workspace, _labels, _no_grad

KMEANS_MAX_K, KMEANS_MAX_CLASSES = 128, 32                  # include/ggan.h: GGAN_KMEANS_MAX_K, GGAN_KMEANS_MAX_CLASSES
KMEANS_ROW_BLOCK, KMEANS_MAX_ROWS, KMEANS_MAX_ITERS = 512, 131072, 1000    # GGAN_KMEANS_ROW_BLOCK, the row range, GGAN_KMEANS_MAX_ITERS
KMEANS_NONFINITE, KMEANS_BAD_INDEX = 1, 2                   # ... and the bits of the status words

KMeansFit = collections.namedtuple('KMeansFit', 'centres idx assign counts inertia moved status')
KMeansFit.__doc__ = """a fitted k-means, device tensors: centres float32 [k, d], idx int32 [k] (the rows the seeding picked), assign int32 [n] and counts
int32 [k] of the final assignment, inertia float64 [iters + 1] and moved int32 [iters + 1] of every assignment (moved[0] = n; moved[-1] == 0:
converged), status int32 [1] (0, or KMEANS_NONFINITE)"""


def _rows(name, x, what='rows'):
    """float32 [1 <= rows <= KMEANS_MAX_ROWS, d >= 1] on the device, no gradient -> contiguous (a view is copied)"""
    _dev(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not 1 <= x.shape[0] <= KMEANS_MAX_ROWS or x.shape[1] < 1:
        raise ValueError('%s: float32 %s [1 <= rows <= %d, d >= 1] expected, got %s %s' % (name, what, KMEANS_MAX_ROWS, x.dtype, tuple(x.shape)))
    _no_grad(name, [x])
    return _c(x)


def _k(name, k):
    k = int(k)
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError('%s: 1 <= k <= %d centres expected, got %d' % (name, KMEANS_MAX_K, k))
    return k


def _uniforms(name, u, k, dev):
    """k uniforms in [0, 1) as a device float64 [k]: a host sequence (uploaded) or a device tensor"""
    if not torch.is_tensor(u):
        u = torch.as_tensor(np.asarray(u, np.float64).reshape(-1))
    if u.dim() != 1 or u.shape[0] != k or u.dtype != torch.float64:
        raise ValueError('%s: %d float64 uniforms expected, got %s %s' % (name, k, u.dtype, tuple(u.shape)))
    return u.to(dev).contiguous()


def _ws(x, k):
    return _workspace(_L().ggan_kmeans_workspace(x.shape[0], x.shape[1], k), x.device)


def kmeans_seed(x, k, u):
    """k-means++ seeding of the rows x float32 [n, d] from k uniforms u (ggan_kmeans_seed): centre 0 is row floor(u[0] n), centre t the first
    row whose running fp64 sum of the smallest squared distances to the centres chosen so far exceeds u[t] * total (total 0: row
    floor(u[t] n)) -> (centres float32 [k, d], idx int32 [k]).  The draws are the caller's; the picks stay on the device."""
    name = 'kmeans_seed'
    x, k = _rows(name, x), _k(name, k)
    u = _uniforms(name, u, k, x.device)
    centres = torch.empty((k, x.shape[1]), dtype=torch.float32, device=x.device)
    idx = torch.empty((k,), dtype=torch.int32, device=x.device)
    ws, nbytes = _ws(x, k)
    check(_L().ggan_kmeans_seed(_p(x), x.shape[0], x.shape[1], k, _p(u), _p(centres), _p(idx), _p(ws), nbytes, _stream()), 'ggan_kmeans_seed')
    return centres, idx


def kmeans_pick(mind, u):
    """the pick of one seeding step alone (ggan_kmeans_pick): the first row whose running fp64 sum of mind float32 [n] exceeds u * total
    -> int32 [1]"""
    name = 'kmeans_pick'
    _dev(mind)
    if mind.dim() != 1 or mind.dtype != torch.float32 or not 1 <= mind.shape[0] <= KMEANS_MAX_ROWS:
        raise ValueError('%s: float32 [1 <= rows <= %d] expected, got %s %s' % (name, KMEANS_MAX_ROWS, mind.dtype, tuple(mind.shape)))
    mind = mind.contiguous()
    u = _uniforms(name, [u] if not torch.is_tensor(u) else u, 1, mind.device)
    idx = torch.empty((1,), dtype=torch.int32, device=mind.device)
    check(_L().ggan_kmeans_pick(_p(mind), mind.shape[0], _p(u), _p(idx), _stream()), 'ggan_kmeans_pick')
    return idx


def kmeans_assign(x, centres, prev=None, counts=None):
    """the nearest centre of every row of x float32 [n, d] among centres float32 [k, d], a tie in distance to the LOWER centre index
    (ggan_kmeans_assign) -> (assign int32 [n], dist float32 [n], inertia float64 [1], moved int32 [1], status int32 [1]): the squared
    distances, their fp64 sum, the rows whose centre differs from prev (int32 [n]; all n without one), and KMEANS_NONFINITE where a row, a
    centre or a distance is not finite (the assignment is then still an index below k).  counts int32 [k]: the rows per centre are ADDED
    to it, so that slabs of one set accumulate."""
    name = 'kmeans_assign'
    x, centres = _rows(name, x), _rows(name, centres, 'centres')
    k = _k(name, centres.shape[0])
    if centres.shape[1] != x.shape[1]:
        raise ValueError('%s: rows of width %d, centres of width %d' % (name, x.shape[1], centres.shape[1]))
    n, dev = x.shape[0], x.device
    if prev is not None:
        prev = _labels(name, 'prev', prev, n, dev)
    if counts is not None and (counts.dim() != 1 or counts.dtype != torch.int32 or counts.shape[0] != k or counts.device != dev
                               or not counts.is_contiguous()):
        raise ValueError('%s: counts must be a contiguous int32 [%d] on %s' % (name, k, dev))
    assign = torch.empty((n,), dtype=torch.int32, device=dev)
    dist = torch.empty((n,), dtype=torch.float32, device=dev)
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    moved, status = torch.empty((1,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    ws, nbytes = _ws(x, k)
    check(_L().ggan_kmeans_assign(_p(x), _p(centres), n, x.shape[1], k, _p(prev), _p(assign), _p(dist), _p(inertia), _p(moved), _p(counts),
                                  _p(status), _p(ws), nbytes, _stream()), 'ggan_kmeans_assign')
    return assign, dist, inertia, moved, status


def kmeans_update(x, assign, centres):
    """centre c = the mean of the rows of x float32 [n, d] with assign == c (ggan_kmeans_update: blocks of KMEANS_ROW_BLOCK rows summed in fp32
    in row order, the blocks in fp64); an empty cluster keeps the centre it had -> (new centres float32 [k, d], counts int32 [k]).  The
    given centres are not written."""
    name = 'kmeans_update'
    x = _rows(name, x)
    centres = _rows(name, centres, 'centres').clone()
    k = _k(name, centres.shape[0])
    if centres.shape[1] != x.shape[1]:
        raise ValueError('%s: rows of width %d, centres of width %d' % (name, x.shape[1], centres.shape[1]))
    assign = _labels(name, 'assign', assign, x.shape[0], x.device)
    counts = torch.empty((k,), dtype=torch.int32, device=x.device)
    ws, nbytes = _ws(x, k)
    check(_L().ggan_kmeans_update(_p(x), _p(assign), x.shape[0], x.shape[1], k, _p(centres), _p(counts), _p(ws), nbytes, _stream()),
          'ggan_kmeans_update')
    return centres, counts


def kmeans_fit(x, k, iters, u):
    """Lloyd's k-means of the rows x float32 [n, d] (ggan_kmeans_fit): kmeans_seed from the k uniforms u, `iters` times (assign, update), a
    final assign -> KMeansFit.  The iteration count is fixed -- stopping early would cost a host synchronisation per iteration --;
    moved[-1] == 0 says it converged.  No host synchronisation."""
    name = 'kmeans_fit'
    x, k, iters = _rows(name, x), _k(name, k), int(iters)
    if not 0 <= iters <= KMEANS_MAX_ITERS:
        raise ValueError('%s: 0 <= iters <= %d expected, got %d' % (name, KMEANS_MAX_ITERS, iters))
    u = _uniforms(name, u, k, x.device)
    (n, d), dev = x.shape, x.device
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    fit = KMeansFit(new((k, d), torch.float32), new((k,), torch.int32), new((n,), torch.int32), new((k,), torch.int32),
                    new((iters + 1,), torch.float64), new((iters + 1,), torch.int32), new((1,), torch.int32))
    ws, nbytes = _ws(x, k)
    check(_L().ggan_kmeans_fit(_p(x), n, d, k, iters, _p(u), _p(fit.centres), _p(fit.idx), _p(fit.assign), _p(fit.counts), _p(fit.inertia),
                               _p(fit.moved), _p(fit.status), _p(ws), nbytes, _stream()), 'ggan_kmeans_fit')
    return fit


def _counts(name, what, t, k=None):
    _dev(t)
    if t.dim() != 1 or t.dtype != torch.int32 or (k is not None and t.shape[0] != k):
        raise ValueError('%s: %s must be int32 [%s], got %s %s' % (name, what, 'k' if k is None else k, t.dtype, tuple(t.shape)))
    return t.contiguous()


def bin_test(counts_ref, counts_test, z_threshold=1.959963984540054):
    """NDB (Richardson & Weiss 2018) of two histograms int32 [k] over the same bins (ggan_bin_test) -> float64 [3] = [the bins whose
    two-proportion z statistic exceeds z_threshold (a bin with a zero standard error does not differ), that number over k, the
    Jensen-Shannon divergence of the two histograms in nats]; all fp64.  An empty histogram gives NaN."""
    name = 'bin_test'
    counts_ref = _counts(name, 'counts_ref', counts_ref)
    k = _k(name, counts_ref.shape[0])
    counts_test = _counts(name, 'counts_test', counts_test, k)
    out = torch.empty((3,), dtype=torch.float64, device=counts_ref.device)
    check(_L().ggan_bin_test(_p(counts_ref), _p(counts_test), k, float(z_threshold), _p(out), _stream()), 'ggan_bin_test')
    return out


def cluster_scores(assign, labels, k, classes):
    """purity and normalised mutual information of an assignment int32 [n] in [0, k) against labels int32 [n] in [0, classes)
    (ggan_cluster_scores) -> (values float64 [2] = [purity: every cluster takes its majority label, NMI = I / ((H(U) + H(V)) / 2), 1 when
    both entropies are 0], table int32 [k, classes], status int32 [1]: 0, or KMEANS_BAD_INDEX for a label or an assignment out of range;
    the values are then NaN).  classes <= KMEANS_MAX_CLASSES."""
    name = 'cluster_scores'
    _dev(assign)
    k, classes = _k(name, k), int(classes)
    if not 1 <= classes <= KMEANS_MAX_CLASSES:
        raise ValueError('%s: 1 <= classes <= %d expected, got %d' % (name, KMEANS_MAX_CLASSES, classes))
    if assign.dim() != 1 or not 1 <= assign.shape[0] <= KMEANS_MAX_ROWS:
        raise ValueError('%s: an assignment int32 [1 <= rows <= %d] expected, got %s' % (name, KMEANS_MAX_ROWS, tuple(assign.shape)))
    n, dev = assign.shape[0], assign.device
    assign, labels = _labels(name, 'assign', assign, n, dev), _labels(name, 'labels', labels, n, dev)
    table = torch.empty((k, classes), dtype=torch.int32, device=dev)
    out = torch.empty((2,), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    check(_L().ggan_cluster_scores(_p(assign), _p(labels), n, k, classes, _p(table), _p(out), _p(status), _stream()), 'ggan_cluster_scores')
    return out, table, status
