"""The least-squares linear probe (include/ggan.h: ggan_probe_*; functional.lsq_probe_fit / lsq_probe_predict) restated in float64 numpy,
stage by stage, the inputs of the tests and the bounds they hold the kernels to.

The definition: mu_j = mean_i z_ij, v_j = mean_i (z_ij - mu_j)^2 as written (two passes), s_j = 1 / sqrt(v_j) or 0 for a constant column,
zs_i = (z_i - mu) * s, G = Zs^T Zs / n, pi_c = n_c / n, R[:, c] = (1/n) sum_{y_i = c} zs_i, W = (G + lambda I)^-1 R,
score(z) = ((z - mu) * s) W + pi, the prediction its argmax with a tie to the lowest class.

The bounds are derived, none is tuned (u = 2^-24, gamma_k = k u / (1 - k u)):
  moments   4 u relative: the sums are accumulated in fp64, so what is left is the one rounding to float32 of mu and of s (u each) and
            the float32 rounding inside 1 / sqrt(v);
  G, R      gamma_B sum|terms| + u |sum|, B = ROW_BLOCK: a block of B rows is summed in fp32 (the textbook forward bound of a sum of B
            products), the block partials in fp64, the result rounded once;
  solve     the residual |(G + lambda I) W - R| of the device's W against the float64 solution of the device's G and R (whose residual is
            nil): 4 u max|R|;
  predict   the device's class equals the float64 argmax from the device's W, mu, s on every row whose float64 top-two margin exceeds
            2 gamma_{d+1} sum_j |zs_j| |W_jc| (the larger of the two classes' sums); at most 2 % of a row's rows may fall below it;
  W         end to end against float64 from the raw inputs: 4 x the error of the float32 numpy restatement fit32 on the same inputs
            (max |W - W64| / max |W64|): the kernels' summation order differs from numpy's, a wrong formula misses by O(1)."""
import functools

import numpy as np

U = 2.0 ** -24
ROW_BLOCK = 256               # GGAN_PROBE_ROW_BLOCK
MAX_DIM, MAX_CLASSES = 128, 32
RIDGE = np.float32(1e-2)      # evaluate.PROBE_RIDGE as the C ABI carries it
BAD_LABEL, NONFINITE, BAD_PIVOT = 1, 2, 4
OPEN_ROWS_CAP = 0.02
W_FACTOR = 4.0
PAD, SENTINEL = 64, -7.5e8


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the definition, float64 ------------------------------------------------------------------------------------------------------------
def moments(Z, y, C):
    Z = np.asarray(Z, np.float64)
    mu = Z.mean(axis=0)
    v = ((Z - mu) ** 2).mean(axis=0)
    s = np.where(v > 0, 1.0 / np.sqrt(np.where(v > 0, v, 1.0)), 0.0)
    return mu, s, np.bincount(np.asarray(y), minlength=C)[:C]


def standardise(Z, mu, s):
    return (np.asarray(Z, np.float64) - np.asarray(mu, np.float64)) * np.asarray(s, np.float64)


def onehot(y, C):
    Y = np.zeros((len(y), C))
    Y[np.arange(len(y)), y] = 1.0
    return Y


def normal(Zs, y, C):
    n = float(Zs.shape[0])
    return Zs.T @ Zs / n, Zs.T @ onehot(y, C) / n


def solve(G, R, ridge):
    G, R = np.asarray(G, np.float64), np.asarray(R, np.float64)
    return np.linalg.solve(G + float(ridge) * np.eye(G.shape[0]), R)


def fit(Z, y, C, ridge=RIDGE):
    mu, s, counts = moments(Z, y, C)
    G, R = normal(standardise(Z, mu, s), y, C)
    return dict(mean=mu, inv_std=s, counts=counts, G=G, R=R, W=solve(G, R, ridge), bias=counts / float(len(y)))


def scores(Z, mu, s, W, bias):
    return standardise(Z, mu, s) @ np.asarray(W, np.float64) + np.asarray(bias, np.float64)


def predict(sc):
    return np.argmax(sc, axis=1)          # (the first maximum: the lowest class on a tie)


def accuracy(Z, y, f):
    return float(np.mean(predict(scores(Z, f['mean'], f['inv_std'], f['W'], f['bias'])) == y))


def lstsq_fit(Z, y, C, ridge=RIDGE):
    """the same classifier as a least-squares problem: min |Zs W + 1 b^T - Y|^2 + n lambda |W|^2, the intercept unpenalised -- the
    augmented system [Zs 1; sqrt(n lambda) I 0] [W; b^T] = [Y; 0] through np.linalg.lstsq -> (W, b)"""
    mu, s, _ = moments(Z, y, C)
    Zs = standardise(Z, mu, s)
    n, d = Zs.shape
    A = np.block([[Zs, np.ones((n, 1))], [np.sqrt(n * float(ridge)) * np.eye(d), np.zeros((d, 1))]])
    B = np.concatenate([onehot(y, C), np.zeros((d, C))])
    X = np.linalg.lstsq(A, B, rcond=None)[0]
    return X[:d], X[d]


def fit32(Z, y, C, ridge=RIDGE):
    """the formula in float32 numpy throughout (what a plain float32 implementation gives): the yardstick of the end-to-end check -> W"""
    f4 = np.float32
    Z = np.asarray(Z, f4)
    n = f4(len(y))
    mu = Z.mean(axis=0, dtype=f4)
    v = ((Z - mu) ** 2).mean(axis=0, dtype=f4)
    s = np.where(v > 0, f4(1) / np.sqrt(np.where(v > 0, v, f4(1))), f4(0)).astype(f4)
    Zs = (Z - mu) * s
    G = (Zs.T @ Zs) / n
    R = (Zs.T @ onehot(y, C).astype(f4)) / n
    return np.linalg.solve(G + f4(ridge) * np.eye(G.shape[0], dtype=f4), R).astype(f4)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
# (n fit rows, m scoring rows, d, C): the issue's five shapes -- d = 1, the MNIST scripts' DIM_LATENT = 8, a width that is no multiple of
# the 32-wide tile, both caps --, one more width so that every instance of the normal-equations kernel (t = ceil(d / 32) = 1 .. 4) runs, and
# the special rows.  sep: the spread of the class means in units of the noise, chosen per row so that the float64 accuracy is neither
# trivial end (asserted in test_probe_cpu on MIDDLE of them).
ROWS = (
    dict(n=64, m=40, d=1, C=2, sep=1.0),
    dict(n=257, m=131, d=8, C=10, sep=0.8),                 # n = one row block + 1
    dict(n=1000, m=300, d=37, C=10, sep=0.35),
    dict(n=1500, m=513, d=128, C=13, sep=0.2),
    dict(n=300, m=100, d=128, C=32, sep=0.35),
    dict(n=600, m=200, d=70, C=10, sep=0.25),               # t = 3
    dict(n=400, m=150, d=8, C=5, sep=0.8, const=3),         # column 3 is constant over the fit rows
    dict(n=500, m=150, d=16, C=6, sep=0.6, absent=4),       # no fit row of class 4
    dict(n=512, m=150, d=16, C=6, sep=0.6, tie=(1, 4)),     # classes 1 and 4 get the same rows, pair by pair: their scores tie exactly
    dict(n=2 * ROW_BLOCK + 1, m=64, d=33, C=7, sep=0.4),    # two full blocks and a block of one row; one column past a tile
)
MIDDLE = (0.5, 0.95)


def row_id(r):
    extra = [k for k in ('const', 'absent', 'tie') if k in r]
    return 'n%d-m%d-d%d-C%d%s' % (r['n'], r['m'], r['d'], r['C'], ('-' + extra[0]) if extra else '')


def instance(r):
    return 'probe_normal_t%d' % ((r['d'] + 31) // 32)


def launches(r):
    """{(profiler label, work-items per launch): launches} of one fit + one prediction of the n fit rows + one of the m scoring rows"""
    n, m, d, C = r['n'], r['m'], r['d'], r['C']
    nb, per = -(-n // ROW_BLOCK), d * d + d * C
    want = {}
    for label, wgs, block in (('probe_colsum', nb, 256), ('probe_mean', 1, 128), ('probe_colsum_sq', nb, 256), ('probe_moments_final', 1, 128),
                              (instance(r), nb, 256), ('probe_normal_combine', -(-per // 256), 256), ('probe_solve', 1, 256),
                              ('probe_predict', -(-n // 64), 256), ('probe_predict', -(-m // 64), 256)):
        want[(label, wgs * block)] = want.get((label, wgs * block), 0) + 1
    return want


@functools.lru_cache(None)
def inputs(idx):
    """row idx of ROWS -> dict(Z [n, d] float32, y [n], Zq [m, d] float32, yq [m]): class means N(0, sep^2) plus unit noise, every column
    then scaled by exp(U(-3, 3)) and offset by U(-50, 50) (a one-pass variance loses its digits on these).  Read-only."""
    r = ROWS[idx]
    n, m, d, C = r['n'], r['m'], r['d'], r['C']
    rng = np.random.default_rng(4200 + idx)
    means = rng.normal(0.0, r['sep'], size=(C, d))
    y = rng.integers(0, C, size=n + m)
    y[:C] = np.arange(C)                                     # (every class is there ...)
    if 'absent' in r:                                        # (... but this one, among the fit rows)
        fit_y = y[:n]
        fit_y[fit_y == r['absent']] = (r['absent'] + 1) % C
    if 'tie' in r:
        a, b = r['tie']
        other = np.array([c for c in range(C) if c not in (a, b)])
        y[:n] = other[rng.integers(0, len(other), size=n)]
        y[0:n // 2:2], y[1:n // 2:2] = a, b                  # rows 2k / 2k + 1 of the first half: a pair
    X = means[y] + rng.normal(size=(n + m, d))
    if 'tie' in r:
        X[1:n // 2:2] = X[0:n // 2:2]
    X = X * np.exp(rng.uniform(-3, 3, size=d)) + rng.uniform(-50, 50, size=d)
    if 'const' in r:
        X[:n, r['const']] = X[0, r['const']]
    Z = X.astype(np.float32)
    out = dict(Z=Z[:n], y=y[:n].astype(np.int32), Zq=Z[n:], yq=y[n:].astype(np.int32))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def reference(idx):
    """the float64 fit of row idx from the raw inputs, its accuracies, and the float32 restatement's error in W"""
    r, x = ROWS[idx], inputs(idx)
    f = fit(x['Z'], x['y'], r['C'])
    f['acc_fit'], f['acc_dev'] = accuracy(x['Z'], x['y'], f), accuracy(x['Zq'], x['yq'], f)
    f['w32_err'] = rel_w(fit32(x['Z'], x['y'], r['C']), f['W'])
    return f


def rel_w(W, W64):
    return float(np.max(np.abs(np.asarray(W, np.float64) - W64)) / np.max(np.abs(W64)))


# ---- the stage checks: each returns the worst observed fraction of its bound ----------------------------------------------------------------
def check_moments(Z, y, C, mean, inv_std, counts):
    mu, s, cnt = moments(Z, y, C)
    assert np.array_equal(np.asarray(counts), cnt), (counts, cnt)
    fm = np.max(np.abs(mean - mu) / (4 * U * np.abs(mu)))
    assert np.array_equal(inv_std == 0, s == 0)
    nz = s > 0
    fs = np.max(np.abs(inv_std[nz] - s[nz]) / (4 * U * s[nz])) if nz.any() else 0.0
    return dict(mean=float(fm), inv_std=float(fs))


def check_normal(Z, y, C, mean, inv_std, G, R):
    """G and R against float64 from the float32 Z, mean, inv_std the kernel read"""
    Zs = standardise(Z, mean, inv_std)
    n = float(len(y))
    G64, R64 = normal(Zs, y, C)
    g = gamma(ROW_BLOCK)
    bG = g * (np.abs(Zs).T @ np.abs(Zs)) / n + U * np.abs(G64)
    bR = g * (np.abs(Zs).T @ onehot(y, C)) / n + U * np.abs(R64)
    zero = lambda b, e: np.all(e[b == 0] == 0)                 # (a bound of 0 -- a constant column, an absent class -- means exactly 0)
    eG, eR = np.abs(G - G64), np.abs(R - R64)
    assert zero(bG, eG) and zero(bR, eR)
    return dict(G=float(np.max(eG[bG > 0] / bG[bG > 0])), R=float(np.max(eR[bR > 0] / bR[bR > 0])))


def check_solve(G, R, W, ridge=RIDGE):
    G, R = np.asarray(G, np.float64), np.asarray(R, np.float64)
    res = (G + float(ridge) * np.eye(G.shape[0])) @ np.asarray(W, np.float64) - R
    return dict(solve=float(np.max(np.abs(res)) / (4 * U * np.max(np.abs(R)))))


def margins(Z, mean, inv_std, W, bias, twin=None):
    """float64 scores from the float32 values the prediction reads -> (the float64 classes, which rows are CLOSED: top-two margin above
    2 gamma_{d+1} sum_j |zs_j| |W_jc|, the larger of the two classes' sums, the scores).  twin = (a, b), a < b: class b's weights and bias
    are bit for bit class a's, so its score IS a's and the tie rule alone keeps it from winning: it is left out of the margin (its score
    set to -inf), and a row where a wins by a clear margin over the REST must come out as a."""
    Zs = standardise(Z, mean, inv_std)
    W = np.asarray(W, np.float64)
    sc = Zs @ W + np.asarray(bias, np.float64)
    mag = np.abs(Zs) @ np.abs(W)
    if twin is not None:
        a, b = twin
        assert a < b and np.array_equal(sc[:, a], sc[:, b])
        sc = sc.copy()
        sc[:, b] = -np.inf
    order = np.argsort(-sc, axis=1, kind='stable')
    rows = np.arange(len(sc))
    if sc.shape[1] == 1:
        return predict(sc), np.ones(len(sc), bool), sc
    top, second = order[:, 0], order[:, 1]
    margin = sc[rows, top] - sc[rows, second]
    bound = 2 * gamma(Z.shape[1] + 1) * np.maximum(mag[rows, top], mag[rows, second])
    return predict(sc), margin > bound, sc
