"""t-SNE on the device (csrc/tsne.hip): what TSNE().fit_transform does on the host in gan_inference_mnist.py:472-480 and
gmgan_inference_mnist.py:533-551.  Forward only; every stage is a function of its own so that the tests can check them one by one:

  tsne_neighbours -> tsne_affinities -> tsne_symmetrise -> tsne_step x n_iter (tsne_gradient: the terms of one gradient; tsne_kl)

The schedule is that of the reference's TSNE(): perplexity 30 over 3 * perplexity neighbours, early exaggeration 12 and momentum 0.5 for
250 iterations, then momentum 0.8 up to 1000, learning rate 200, Y0 = 1e-4 * N(0, 1).  Three deliberate differences: the repulsive term is
summed exactly over all pairs (no Barnes-Hut tree); the iteration count is fixed (no early stop on stalled progress); and the bisection on
beta works on distances relative to each row's nearest neighbour, so the row sum needs no floor (scikit-learn floors it at 1e-8, which
binds where beta times the nearest distance exceeds about 18 and then leaves that row away from the target perplexity)."""
import numpy as np
import torch

from .. import _lib
from ._core import _L, _c, _dev, _p, _stream, check, workspace

TSNE_BLOCK_BYTES = 64 << 20        # the distance block of tsne_neighbours: rows * N floats at a time, never the whole N x N matrix
MOMENTUM = (0.5, 0.8)
MIN_GAIN = 0.01


def tsne_splits(N):
    """the default cut of the j range of the repulsive sum: enough workgroups of 256 points x one split to give each of the chip's
    1024 SIMDs four wavefronts, at most 64 splits (one lane of the combining wavefront each)"""
    return int(max(1, min(_lib.TSNE_MAX_SPLITS, -(-1024 // -(-int(N) // 256)))))


def tsne_neighbours(X, K, block_rows=None):
    """X [N, D] -> (idx int32 [N, K], dist float32 [N, K]): the K nearest other rows in squared Euclidean distance, ascending; a tie in
    distance goes to the lower index.  The distances are |x_i|^2 + |x_j|^2 - 2 x_i.x_j with the products from ggan_gemm, a block of
    rows at a time."""
    X = _c(X)
    N, D = X.shape
    K = int(K)
    rows = int(block_rows) if block_rows else max(1, min(N, TSNE_BLOCK_BYTES // (4 * N)))
    ws = workspace(X.device)
    norms = torch.empty((N,), dtype=torch.float32, device=X.device)
    dots = torch.empty((rows, N), dtype=torch.float32, device=X.device)
    idx = torch.empty((N, K), dtype=torch.int32, device=X.device)
    dist = torch.empty((N, K), dtype=torch.float32, device=X.device)
    check(_L().ggan_tsne_sqnorms(_p(X), N, D, _p(norms), _stream()), 'ggan_tsne_sqnorms')
    for r0 in range(0, N, rows):
        check(_L().ggan_tsne_neighbours(_p(X), _p(norms), N, D, r0, min(rows, N - r0), K, _p(dots), _p(idx), _p(dist), _p(ws), ws.numel(),
                                        _stream()), 'ggan_tsne_neighbours')
    return idx, dist


def tsne_affinities(dist, perplexity=30., steps=100, tol=1e-5):
    """dist [N, K] -> (p_cond [N, K], beta [N]): p_j|i = exp(-beta_i d_ij) / sum over the K neighbours, beta_i from the reference's
    bisection (from 1, at most `steps` steps, until the entropy is log(perplexity) within tol).  Each row of dist must be ascending, as
    tsne_neighbours returns it: the kernel takes the distances relative to the row's first entry (p and the entropy do not change, and
    unlike scikit-learn no floor on the row sum is needed)."""
    dist = _c(dist)
    N, K = dist.shape
    p = torch.empty_like(dist)
    beta = torch.empty((N,), dtype=torch.float32, device=dist.device)
    check(_L().ggan_tsne_affinities(_p(dist), N, K, float(perplexity), int(steps), float(tol), _p(p), _p(beta), _stream()), 'ggan_tsne_affinities')
    return p, beta


def tsne_symmetrise(idx, p_cond):
    """-> (ptr int32 [N + 1], col int32 [2 N K], val float32 [2 N K]): P = (P + P^T) / 2N as a CSR.  Row i: its K neighbours in their
    order, then every j whose list holds i, ascending; a j in both groups has its whole value in the first and 0 in the second."""
    p_cond = _c(p_cond)
    _dev(idx)
    N, K = p_cond.shape
    assert idx.dtype == torch.int32 and idx.is_contiguous() and tuple(idx.shape) == (N, K), (idx.dtype, idx.shape)
    dev = idx.device
    ptr = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    col = torch.empty((2 * N * K,), dtype=torch.int32, device=dev)
    val = torch.empty((2 * N * K,), dtype=torch.float32, device=dev)
    scratch = torch.empty((2 * N + N * K,), dtype=torch.int32, device=dev)
    check(_L().ggan_tsne_symmetrise(_p(idx), _p(p_cond), N, K, _p(ptr), _p(col), _p(val), _p(scratch), _stream()), 'ggan_tsne_symmetrise')
    return ptr, col, val


def _partials(N, splits, dev):
    return (torch.empty((splits * 2 * N,), dtype=torch.float32, device=dev),
            torch.empty((splits * (-(-N // 256)),), dtype=torch.float32, device=dev))


def _embedding(P, Y):
    ptr, col, val = P
    Y = _c(Y)
    N = Y.shape[0]
    assert tuple(Y.shape) == (N, 2) and ptr.numel() == N + 1 and ptr.dtype == torch.int32 and col.dtype == torch.int32, (Y.shape, ptr.shape)
    _c(val)
    return ptr, col, val, Y, N


def tsne_gradient(P, Y, splits=None):
    """the terms of one gradient at Y [N, 2] -> (attr [N, 2] = sum_j P_ij q_ij (y_i - y_j), rep [N, 2] = sum_j q_ij^2 (y_i - y_j),
    Z [1] = sum_{i != j} q_ij); grad = 4 (exaggeration * attr - rep / Z)"""
    ptr, col, val, Y, N = _embedding(P, Y)
    splits = int(splits or tsne_splits(N))
    part, zblk = _partials(N, splits, Y.device)
    attr, rep = torch.empty_like(Y), torch.empty_like(Y)
    z = torch.empty((1,), dtype=torch.float32, device=Y.device)
    check(_L().ggan_tsne_gradient(_p(ptr), _p(col), _p(val), _p(Y), N, splits, _p(part), _p(zblk), _p(attr), _p(rep), _p(z), _stream()),
          'ggan_tsne_gradient')
    return attr, rep, z


def tsne_kl(P, Y, splits=None):
    """KL(P || Q) of the embedding Y under the sparse P -> float32 [1] on the device"""
    ptr, col, val, Y, N = _embedding(P, Y)
    splits = int(splits or tsne_splits(N))
    part, zblk = _partials(N, splits, Y.device)
    klrow = torch.empty((N,), dtype=torch.float32, device=Y.device)
    kl = torch.empty((1,), dtype=torch.float32, device=Y.device)
    check(_L().ggan_tsne_kl(_p(ptr), _p(col), _p(val), _p(Y), N, splits, _p(part), _p(zblk), _p(klrow), _p(kl), _stream()), 'ggan_tsne_kl')
    return kl


def tsne_step(P, Y, vel, gains, it0=0, n=1, learning_rate=200., early_exaggeration=12., exploration_iters=250, splits=None):
    """iterations it0 .. it0 + n - 1 of the descent from Y -> the new Y [N, 2]; vel and gains [N, 2] are updated in place, Y is left
    as it was only when n is 0 (it is one of the two position buffers the iterations alternate between)"""
    ptr, col, val, Y, N = _embedding(P, Y)
    for t in (vel, gains):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N, 2), t.shape
        _dev(t)
    splits = int(splits or tsne_splits(N))
    part, zblk = _partials(N, splits, Y.device)
    other = torch.empty_like(Y)
    check(_L().ggan_tsne_iterate(_p(ptr), _p(col), _p(val), _p(Y), _p(other), _p(vel), _p(gains), N, splits, _p(part), _p(zblk), int(it0),
                                 int(it0) + int(n), int(exploration_iters), float(early_exaggeration), MOMENTUM[0], MOMENTUM[1],
                                 float(learning_rate), MIN_GAIN, _stream()), 'ggan_tsne_iterate')
    return other if n % 2 else Y


def tsne_affinity_graph(X, perplexity=30.):
    """X [N, D] -> the symmetrised P (ptr, col, val) over K = 3 * perplexity neighbours"""
    N = X.shape[0]
    if not perplexity < N:
        raise _lib.GganError('tsne: perplexity %g needs more than %d points' % (perplexity, N))
    K = int(min(N - 1, 3. * perplexity))
    if K > _lib.TSNE_MAX_K:
        raise _lib.GganError('tsne: perplexity %g asks for %d neighbours, the kernels keep at most %d' % (perplexity, K, _lib.TSNE_MAX_K))
    idx, dist = tsne_neighbours(X, K)
    p_cond, _ = tsne_affinities(dist, perplexity)
    return tsne_symmetrise(idx, p_cond)


def tsne(X, perplexity=30., n_iter=1000, learning_rate=200., early_exaggeration=12., exploration_iters=250, seed=0, y0=None,
         return_kl=False, splits=None):
    """X [N, D] on the device -> Y [N, 2] (and KL(P || Q) of it as a float with return_kl).  y0: the initial embedding; by default
    1e-4 * RandomState(seed).standard_normal((N, 2)), drawn from a generator of its own (numpy's global stream is not consumed)."""
    X = _c(X)
    N = X.shape[0]
    P = tsne_affinity_graph(X, perplexity)
    if y0 is None:
        y0 = torch.as_tensor((1e-4 * np.random.RandomState(seed).standard_normal((N, 2))).astype(np.float32))
    Y = _c(y0.to(X.device, torch.float32)).clone()
    assert tuple(Y.shape) == (N, 2), Y.shape
    vel, gains = torch.zeros_like(Y), torch.ones_like(Y)
    Y = tsne_step(P, Y, vel, gains, 0, int(n_iter), learning_rate, early_exaggeration, exploration_iters, splits)
    if return_kl:
        return Y, float(tsne_kl(P, Y, splits).item())
    return Y
