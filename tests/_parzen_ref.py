"""The float64 restatement the Parzen-window tests hold the device to (ggan_parzen_lse, functional.parzen_lse / parzen_ll,
Evaluator.parzen_scores): squared distances by DIRECT differences -- no Gram trick --, the log-sum-exp in its shifted form, the
log-likelihood in the unit-interval pixel scale, the choice of the bandwidth and the three values of the pass; plus the cached, read-only
recipes of the cases that tests/test_parzen_cpu.py and tests/test_parzen_gpu.py share.

The gate is the project's one for set-level values (tests/test_mmd_sets_gpu.py): |got - ref| <= 2e-5 max(1, |ref|), per row and bandwidth."""
import functools

import numpy as np

GATE = 2e-5
SIGMAS = np.logspace(-1, 0, 10)                  # evaluate.PARZEN_SIGMAS, restated (test_parzen_cpu compares the two)
LATTICE_CASES = [(2, 1, 1), (5, 9, 16), (130, 67, 33), (257, 300, 131), (192, 160, 3072)]
LATTICE_FACTORS = (0.05, 0.2, 1.0, 30.0)         # times sqrt(4 d): from nearest-neighbour-only up to every-candidate-counts
IMAGE_CASES = [(130, 300, 784), (64, 200, 3072)]


def gate(ref):
    return GATE * np.maximum(1.0, np.abs(ref))


def d2(Q, S):
    """squared distances [m, n] in float64 from direct differences, a block of queries at a time"""
    Q, S = np.asarray(Q, np.float64), np.asarray(S, np.float64)
    out = np.empty((Q.shape[0], S.shape[0]))
    step = max(1, (1 << 24) // max(1, S.shape[0] * S.shape[1]))
    for i in range(0, Q.shape[0], step):
        diff = Q[i:i + step, None, :] - S[None, :, :]
        out[i:i + step] = np.einsum('ijk,ijk->ij', diff, diff)
    return out


def lse_from_d2(D, sigmas):
    """[ns, m]: log sum_j exp(-D[i, j] / (2 sigma^2)), shifted by the row's minimum distance"""
    D = np.asarray(D, np.float64)
    dmin = D.min(axis=1)
    out = []
    for s in np.asarray(sigmas, np.float64).reshape(-1):
        c = 1.0 / (2.0 * s * s)
        out.append(np.log(np.exp(-(D - dmin[:, None]) * c).sum(axis=1)) - dmin * c)
    return np.stack(out)


def lse(Q, S, sigmas):
    return lse_from_d2(d2(Q, S), sigmas)


def plain_lse(D, sigmas):
    """the sum that is NOT shifted, in float64: what underflows to log 0 at image bandwidths"""
    with np.errstate(divide='ignore'):
        return np.stack([np.log(np.exp(-np.asarray(D, np.float64) / (2.0 * s * s)).sum(axis=1)) for s in np.asarray(sigmas, np.float64).reshape(-1)])


def ll(Q, S, sigmas, scale=1.0):
    """[ns, m]: the Parzen log-likelihood per row in the unit-interval pixel scale, rows handed in `scale` times as wide:
    lse(scale sigma) - log n - (d / 2) log(2 pi sigma^2)"""
    sig = np.asarray(sigmas, np.float64).reshape(-1)
    n, d = np.asarray(S).shape
    return lse(Q, S, scale * sig) - np.log(n) - 0.5 * d * np.log(2.0 * np.pi * sig * sig)[:, None]


def valid_rows(rows, B, valid=1000):
    """the leading rows the bandwidth is chosen on: whole minibatches, at most `valid` rows and at most half the minibatches, at least one"""
    return B * max(1, min(valid // B, (rows // B) // 2))


def pass_values(x, gx, B, sigmas=SIGMAS, scale=1.0, valid=1000):
    """the three values of the pass from the sets it built, and what the tests need beside them"""
    sig = np.asarray(sigmas, np.float64).reshape(-1)
    L = ll(x, gx, sig, scale)
    v = valid_rows(L.shape[1], B, valid)
    means = L[:, :v].mean(axis=1)
    best = int(np.argmax(means))                        # (numpy's argmax is the first of equal values)
    held = L[best, v:]
    return dict(ll=float(held.mean()), se=float(held.std() / np.sqrt(len(held))), sigma=float(sig[best]), best=best, valid_means=means,
                rows=L, v=v, count=len(held))


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def lattice(m, n, d):
    """(Q, S, sigmas): integer coordinates in -2 .. 2 -- every norm and dot product is exact in float32, so D is, and only the exp / log
    arithmetic is under test --, the first min(m, n) // 3 rows of S copies of rows of Q (exact zeros)"""
    rng = np.random.default_rng(1000 * m + 10 * n + d)
    Q = rng.integers(-2, 3, size=(m, d)).astype(np.float32)
    S = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    c = min(m, n) // 3
    S[:c] = Q[rng.permutation(m)[:c]]
    sig = np.array(LATTICE_FACTORS) * np.sqrt(4.0 * d)
    return _frozen(Q, S, sig)


@functools.lru_cache(maxsize=None)
def image_like(m, n, d):
    """(Q, S, sigmas): d = 784: rows u^3 in [0, 1), the pass's own bandwidths; d = 3072: rows 2 u^2 - 1 in [-1, 1), twice those"""
    rng = np.random.default_rng(7 * m + n + d)
    f = (lambda u: u ** 3) if d == 784 else (lambda u: 2.0 * u ** 2 - 1.0)
    Q, S = f(rng.random((m, d))).astype(np.float32), f(rng.random((n, d))).astype(np.float32)
    sig = np.array(SIGMAS if d == 784 else 2.0 * SIGMAS)
    return _frozen(Q, S, sig)


def case(m, n, d):
    return lattice(m, n, d) if (m, n, d) in LATTICE_CASES else image_like(m, n, d)


@functools.lru_cache(maxsize=None)
def case_d2(m, n, d):
    Q, S, _ = case(m, n, d)
    return _frozen(d2(Q, S))[0]


@functools.lru_cache(maxsize=None)
def reference(m, n, d):
    """lse [ns, m] of a shared case"""
    return _frozen(lse_from_d2(case_d2(m, n, d), case(m, n, d)[2]))[0]
