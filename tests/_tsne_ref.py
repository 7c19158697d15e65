"""float64 numpy restatement of the stages of functional/tsne.py (csrc/tsne.hip), for the t-SNE tests and the fixture generator:
neighbours, the bisection on beta, symmetrise, the exact gradient, one update, KL_s.  Dense [N, N] arrays: meant for N of a
thousand or so."""
import numpy as np

MOMENTUM = (0.5, 0.8)


def fixture_inputs(recipe):
    """the recipe of tests/golden/tsne_reference.json -> (X float32 [N, D], labels [N])"""
    rng = np.random.RandomState(recipe['seed'])
    K, D, n = recipe['clusters'], recipe['dim'], recipe['per_cluster']
    mu = rng.normal(size=(K, D)) * recipe['centre_scale']
    X = (mu[:, None, :] + rng.normal(size=(K, n, D))).reshape(-1, D).astype(np.float32)
    return X, np.repeat(np.arange(K), n)


def sq_distances(X):
    """[N, N] squared Euclidean distances in float64 (direct form up to 4000 points), +inf on the diagonal"""
    X = np.asarray(X, np.float64)
    if len(X) <= 4000:
        d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    else:
        n = (X ** 2).sum(1)
        d = np.maximum(n[:, None] + n[None, :] - 2.0 * (X @ X.T), 0.0)
    np.fill_diagonal(d, np.inf)
    return d


def neighbours(X, K, d=None):
    """-> (idx [N, K], dist [N, K]): ascending in (distance, index)"""
    d = sq_distances(X) if d is None else d
    idx = np.argsort(d, 1, kind='stable')[:, :K]
    return idx, np.take_along_axis(d, idx, 1)


def entropy(dist, beta):
    """the entropy of p_j|i = exp(-beta_i d_ij) / sum, per row (natural log), and p"""
    dist, beta = np.asarray(dist, np.float64), np.asarray(beta, np.float64).reshape(-1, 1)
    rel = dist - dist.min(1, keepdims=True)             # (p and the entropy do not depend on the shift)
    p = np.exp(-rel * beta)
    s = p.sum(1, keepdims=True)
    p = p / s
    return np.log(s[:, 0]) + beta[:, 0] * (rel * p).sum(1), p


def affinities(dist, perplexity=30., steps=100, tol=1e-5):
    """sklearn's _binary_search_perplexity -> (p_cond [N, K], beta [N]: the value p_cond was formed with).  One difference: the
    distances of a row are taken relative to its smallest.  p and the entropy are the same function of beta either way; sklearn
    works on the raw distances and floors sum_j exp(-beta d_ij) at 1e-8, which binds once beta * d_i1 exceeds about 18 (perplexity 5 on
    the awkward shape of the GPU tests does that) and then stops the search at a beta whose entropy is NOT log(perplexity).  With
    relative distances the sum is at least 1 and the floor never binds; on the fixture inputs it does not bind in sklearn either."""
    dist = np.asarray(dist, np.float64)
    dist = dist - dist.min(1, keepdims=True)
    N = len(dist)
    H = np.log(perplexity)
    P, betas = np.zeros_like(dist), np.zeros(N)
    for i in range(N):
        lo, hi, b = -np.inf, np.inf, 1.0
        for _ in range(steps):
            p = np.exp(-dist[i] * b)
            s = p.sum()
            p = p / s
            h = np.log(s) + b * (dist[i] * p).sum()
            used = b
            if abs(h - H) <= tol:
                break
            if h > H:
                lo = b
                b = b * 2 if hi == np.inf else (b + hi) / 2
            else:
                hi = b
                b = b / 2 if lo == -np.inf else (b + lo) / 2
        P[i], betas[i] = p, used
    return P, betas


def symmetrise(idx, p_cond):
    """-> dense P [N, N] = (P + P^T) / 2N"""
    N = len(idx)
    P = np.zeros((N, N))
    np.put_along_axis(P, np.asarray(idx, np.int64), np.asarray(p_cond, np.float64), 1)
    return (P + P.T) / (2.0 * N)


def sparse_P(X, perplexity=30.):
    X = np.asarray(X)
    K = int(min(len(X) - 1, 3. * perplexity))
    idx, dist = neighbours(X, K)
    return symmetrise(idx, affinities(dist, perplexity)[0])


def gradient_terms(P, Y):
    """-> (attr [N, 2] = sum_j P_ij q_ij (y_i - y_j), rep [N, 2] = sum_j q_ij^2 (y_i - y_j), Z)"""
    Y = np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    attr = ((P * q)[:, :, None] * diff).sum(1)
    rep = ((q * q)[:, :, None] * diff).sum(1)
    return attr, rep, q.sum()


def update(P, Y, V, G, it, learning_rate=200., early_exaggeration=12., exploration_iters=250, min_gain=0.01):
    """iteration `it` -> (Y, V, G) after it"""
    e, mom = (early_exaggeration, MOMENTUM[0]) if it < exploration_iters else (1.0, MOMENTUM[1])
    attr, rep, Z = gradient_terms(P, Y)
    g = 4.0 * (e * attr - rep / Z)
    G = np.maximum(np.where(V * g < 0, G + 0.2, G * 0.8), min_gain)
    V = mom * V - learning_rate * G * g
    return Y + V, V, G


def initial(N, seed):
    return 1e-4 * np.random.RandomState(seed).standard_normal((N, 2))


def run(P, Y, n_iter=1000, keep=(), **kw):
    """n_iter updates from Y -> (Y, {it: Y after iteration number it, counted from 1} for it in keep)"""
    Y = np.array(Y, np.float64)
    V, G, kept = np.zeros_like(Y), np.ones_like(Y), {}
    for it in range(n_iter):
        Y, V, G = update(P, Y, V, G, it, **kw)
        if it + 1 in keep:
            kept[it + 1] = Y.copy()
    return Y, kept


def kl_sparse(P, Y):
    """KL_s: the KL divergence of the embedding Y under the sparse P, with the exact Z"""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    q = 1.0 / (1.0 + d)
    np.fill_diagonal(q, 0.0)
    Q = np.maximum(q / q.sum(), 1e-300)
    m = P > 0
    return float((P[m] * np.log(P[m] / Q[m])).sum())


def purity(Y, labels, k=10):
    """the share of each point's k nearest neighbours in the embedding that carry its label"""
    idx, _ = neighbours(np.asarray(Y, np.float64), k)
    return float(np.mean(labels[idx] == labels[:, None]))
