"""The wide least-squares probe (include/ggan.h: ggan_wprobe_*; functional.lsq_probe_fit_wide / lsq_probe_predict_wide): the rows of its
tests, its launch plan restated, and the bounds the kernels are held to.  The float64 definition, gamma, the pads and the status bits are
tests/_probe_ref.py's (P below); nothing of them is restated here.

The bounds are derived, none is tuned (u = 2^-24, u64 = 2^-53, gamma_k = k u / (1 - k u), gamma64_k the same with u64):
  moments   4 u relative, as P: fp64 sums, one rounding each of mean and 1 / std;
  G, R      gamma_B sum|terms|, B = ROW_BLOCK: a block of B rows is summed in fp32, the blocks in fp64; the outputs are fp64, so P's final
            u |sum| is gone;
  factor    |L L^T - (G + ridge I)| <= gamma64_{d+1} |L| |L^T| elementwise on the lower triangle: the backward bound of Cholesky
            (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.3), which holds for any order of the inner sums;
  solve     the residual |(G + ridge I) W - R| of the device's float32 W against the device's G and R:
            u |G + ridge I| |W| (the one rounding of W to float32) + gamma64_{3d+1} |L| |L^T| |W| (the two substitutions, Theorem 10.4);
  predict   the device's class equals the float64 argmax from the device's W, mu, s on every row whose float64 top-two margin exceeds
            2 gamma_{CHUNK+1} sum_j |zs_j| |W_jc|: a score is fp32 chains of at most CHUNK columns added in fp64, whatever d is; at most
            P.OPEN_ROWS_CAP of a row's rows may fall below it (the float64 reference alone leaves at most half of that: test_wprobe_cpu);
  W         end to end against float64 from the raw inputs: P.W_FACTOR x the error of P.fit32 on the same inputs."""
import functools

import numpy as np

import _probe_ref as P

U64 = 2.0 ** -53
MAX_DIM, TILE, NB, CHUNK = 4096, 64, 64, 128      # GGAN_WPROBE_MAX_DIM / _TILE / _PANEL / _CHUNK


def gamma64(k):
    return k * U64 / (1.0 - k * U64)


# (n fit rows, m scoring rows, d, C): the smallest shapes at which the kernels can still go wrong
ROWS = (
    dict(n=300, m=100, d=129, C=10),                        # the first width the narrow chain refuses; one padded tile column; a full row block and a partial one
    dict(n=512, m=128, d=4 * NB, C=32),                     # exact tiles, exact panels, exact row blocks, the class cap
    dict(n=150, m=70, d=200, C=3, const=5, absent=2, tie=(0, 1)),      # n < d: only the ridge makes G + ridge I definite; see inputs()
    dict(n=1300, m=200, d=8 * NB + 8, C=32),                # 8 trailing updates over up to 36 tiles; a remainder panel of 8; 5 row blocks and a partial one
    dict(n=700, m=150, d=96, C=10, narrow=True),            # a narrow shape: the wide chain beside ggan_probe_* on the same input
)


def row_id(r):
    extra = [k for k in ('tie', 'narrow') if k in r]
    return 'n%d-m%d-d%d-C%d%s' % (r['n'], r['m'], r['d'], r['C'], ('-' + extra[0]) if extra else '')


def tri(t):
    return t * (t + 1) // 2


def factor_launches(d):
    """[(profiler label, work-items)] of ggan_wprobe_factor, panel by panel"""
    out = []
    for p in range(0, d, NB):
        out.append(('wprobe_chol_diag_nb%d' % NB, NB))
        below = d - p - NB
        if below <= 0:
            break
        nt = -(-below // NB)
        out += [('wprobe_chol_panel_nb%d' % NB, -(-below // NB) * NB), ('wprobe_chol_trail_nb%d' % NB, tri(nt) * 256)]
    return out


def launches(r):
    """{(profiler label, work-items per launch): launches} of one fit + one prediction of the n fit rows + one of the m scoring rows"""
    n, m, d, C = r['n'], r['m'], r['d'], r['C']
    nb, cb, nt = -(-n // P.ROW_BLOCK), -(-d // 256), -(-d // TILE)
    plan = [('wprobe_colsum', nb * cb * 256), ('wprobe_mean', cb * 256), ('wprobe_colsum_sq', nb * cb * 256), ('wprobe_moments_final', cb * 256),
            ('wprobe_normal_t%d' % TILE, (tri(nt) + nt) * 256)] + factor_launches(d)
    plan += [('wprobe_solve_nb%d' % NB, C * 256), ('wprobe_predict_c%d' % CHUNK, -(-n // 64) * 256), ('wprobe_predict_c%d' % CHUNK, -(-m // 64) * 256)]
    want = {}
    for key in plan:
        want[key] = want.get(key, 0) + 1
    return want


@functools.lru_cache(None)
def inputs(idx):
    """row idx of ROWS -> dict(Z [n, d] float32, y [n], Zq [m, d] float32, yq [m]): class means 0.35 N(0, 1) per column plus unit noise,
    the column scales cycling through 1 .. 7, and 10.0 added to everything (a one-pass variance loses its digits on these).  Read-only.
    The row with three classes has them all special: 0 and 1 are twins (the fit rows come in identical pairs, one of each), 2 has no fit
    row.  Its R is then half the column sums of the standardised rows, which are nil: W64 is rounding dust there, and what the row checks
    is the chain at n < d, the exact tie and the zero column -- its end-to-end figure is the device's dust over the float32 restatement's
    (the normaliser max |W64| cancels in the fraction), held to the same W_FACTOR."""
    r = ROWS[idx]
    n, m, d, C = r['n'], r['m'], r['d'], r['C']
    rng = np.random.default_rng(9100 + idx)
    means = 0.35 * rng.normal(size=(C, d))
    y = rng.integers(0, C, size=n + m)
    y[:C] = np.arange(C)
    if 'tie' in r:
        a, b = r['tie']
        assert n % 2 == 0 and sorted((a, b, r['absent'])) == list(range(C))
        y[0:n:2], y[1:n:2] = a, b
    X = means[y] + rng.normal(size=(n + m, d))
    if 'tie' in r:
        X[1:n:2] = X[0:n:2]
    X = X * (1.0 + np.arange(d) % 7) + 10.0
    if 'const' in r:
        X[:n, r['const']] = X[0, r['const']]
    Z = X.astype(np.float32)
    out = dict(Z=Z[:n], y=y[:n].astype(np.int32), Zq=Z[n:], yq=y[n:].astype(np.int32))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def reference(idx):
    """the float64 fit of row idx from the raw inputs (P.fit) and the float32 restatement's error in W"""
    r, x = ROWS[idx], inputs(idx)
    f = P.fit(x['Z'], x['y'], r['C'])
    f['w32_err'] = P.rel_w(P.fit32(x['Z'], x['y'], r['C']), f['W'])
    return f


# ---- the stage checks: each returns the worst observed fraction of its bound ----------------------------------------------------------------
def _worst(err, bound):
    """max err / bound; where the bound is 0 the error must be exactly 0"""
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def check_normal(Z, y, C, mean, inv_std, G, R):
    """the fp64 G and R against float64 from the float32 Z, mean, inv_std the kernel read"""
    Zs = P.standardise(Z, mean, inv_std)
    n = float(len(y))
    G64, R64 = P.normal(Zs, y, C)
    g = P.gamma(P.ROW_BLOCK)
    bG = g * (np.abs(Zs).T @ np.abs(Zs)) / n
    bR = g * (np.abs(Zs).T @ P.onehot(y, C)) / n
    return dict(G=_worst(np.abs(G - G64), bG), R=_worst(np.abs(R - R64), bR))


def check_factor(G, L, ridge=P.RIDGE):
    """the lower triangle L the device left in G's place against the G it was given; the product in extended precision where numpy has it"""
    d = G.shape[0]
    ld = np.longdouble
    A = np.asarray(G, np.float64) + float(ridge) * np.eye(d)
    Lt = np.tril(np.asarray(L, np.float64))
    err = np.abs(np.asarray(Lt.astype(ld) @ Lt.astype(ld).T - A.astype(ld), np.float64))
    bound = gamma64(d + 1) * (np.abs(Lt) @ np.abs(Lt).T)
    low = np.tril(np.ones((d, d), bool))
    return dict(factor=_worst(err[low], bound[low]))


def check_solve(G, R, L, W, ridge=P.RIDGE):
    d = G.shape[0]
    A = np.asarray(G, np.float64) + float(ridge) * np.eye(d)
    Lt = np.tril(np.asarray(L, np.float64))
    W = np.asarray(W, np.float64)
    res = np.abs(A @ W - np.asarray(R, np.float64))
    bound = P.U * (np.abs(A) @ np.abs(W)) + gamma64(3 * d + 1) * ((np.abs(Lt) @ np.abs(Lt).T) @ np.abs(W))
    return dict(solve=_worst(res, bound))


def margins(Z, mean, inv_std, W, bias, twin=None, k=CHUNK + 1):
    """P.margins with the chain length k of the bound a parameter -> (the float64 classes, which rows are CLOSED, the scores, the margins)"""
    Zs = P.standardise(Z, mean, inv_std)
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
    top, second = order[:, 0], order[:, 1]
    margin = sc[rows, top] - sc[rows, second]
    bound = 2 * P.gamma(k) * np.maximum(mag[rows, top], mag[rows, second])
    return P.predict(sc), margin > bound, sc, margin
