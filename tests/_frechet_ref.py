"""The Frechet distance between Gaussians fitted to two row sets, in float64 numpy, for tests/test_frechet_cpu.py and tests/test_frechet_gpu.py:
  reference(x, y)       the yardstick: mean, covariance over n - 1, r = S1^(1/2) by eigh with the eigenvalues clipped at 0, and
                        tr (S1 S2)^(1/2) = sum sqrt(clip(eigvalsh(r S2 r), 0)) -- the symmetric square root, NOT the kernel's route;
  model_distance(...)   the kernel's own route in float64: a diagonally pivoted Cholesky factorisation that tolerates a semi-definite S1 (once the
                        largest remaining pivot is at or below d eps tr S1 the remaining columns are zero), M = L^T S2 L, two-sided Jacobi rotations in round-robin ordering (d / 2 disjoint
                        pairs per step, d - 1 steps per sweep), the off-diagonal norm measured against ||M||_F at the start.  It gives the
                        sweep cap of csrc/frechet.hip and what the fp64 stage can be expected to show;
  the grid and the sets the GPU tests run, and the measured bounds."""
import functools
import zlib

import numpy as np

MAX_DIM, MAX_ROWS, ROW_BLOCK = 128, 131072, 256      # include/ggan.h: GGAN_FRECHET_MAX_DIM, the row range, the probe's row block
NONFINITE, NOT_CONVERGED = 1, 2                       # ... and the bits of the status word
EPS = 2.0 ** -52
U32 = 2.0 ** -24

JACOBI_TOL = 1e-14          # off(M)_F <= JACOBI_TOL ||M at the start||_F ends the iteration (csrc/frechet.hip: kTol)
# the largest number of sweeps model_distance took over cases() (test_frechet_cpu.py::test_the_model_matches_the_reference_and_converges_within_the_cap measures it
# again), and the kernel's fixed trip count: twice that
SWEEPS_SEEN = 10
SWEEP_CAP = 2 * SWEEPS_SEEN

DIMS = (1, 2, 31, 33, 64, 127, 128)
ROWS = (2, 255, 256, 257, 600)                        # one short block, the block edge on both sides, three blocks
KINDS = ('gauss', 'self', 'shift', 'short', 'const', 'twin', 'scale')

# The two gates of the GPU tests, abs(fd - reference) / (tr S1 + tr S2 + |dmu|^2).  Each bound is four times the largest value measured
# over cases() on one MI355X (the margin covers the difference between the grid and what a run meets).  Measured 2026-10-20 on the commit
# that adds the op (parent cd986c6).
FP64_STAGE_SEEN = 3.220e-07     # (a) ggan_frechet_distance fed numpy's float64 moments: 'self' n = 2 d = 127 -- the REFERENCE's error at rank 1
FP64_STAGE_BOUND = 4 * FP64_STAGE_SEEN      # (the float64 model of the kernel's route shows the same 3.22e-07 there and 1e-16 against the exact 0)
WHOLE_OP_SEEN = 1.376e-06       # (b) functional.frechet_distance from the float32 rows: 'short' n = 600 d = 127 (fp32_moments + the model: 1.38e-06)
WHOLE_OP_BOUND = 4 * WHOLE_OP_SEEN
WHOLE_OP_CEILING = ROW_BLOCK * U32      # all an fp32 sum over a block of 256 rows can explain: (b) above it is a bug, not a tolerance


def case_id(kind, n, d):
    return '%s-n%d-d%d' % (kind, n, d)


def cases(kinds=KINDS):
    """(kind, n, d) over the grid; 'twin' needs two columns, 'short' (n < d) three"""
    return [(k, n, d) for k in kinds for d in DIMS for n in ROWS if not (k == 'twin' and d < 2) and not (k == 'short' and d < 3)]


def _gauss(rng, n, d, scale, offset):
    """n float64 rows of a correlated Gaussian: a random mixing of the columns, a scale and a mean of their own"""
    A = rng.normal(size=(d, d)) / np.sqrt(d) + 0.5 * np.eye(d)
    return (rng.normal(size=(n, d)) @ A) * scale + (rng.normal(size=d) * 0.5 + offset)


@functools.lru_cache(None)
def sets(kind, n, d):
    """the two float32 row sets of a case (read-only):
    gauss  correlated Gaussians of unequal scale and mean      self   a set against itself        shift  a set against itself shifted
    short  n < d: both sets cut to max(2, d // 2) rows         const  one constant column in both twin   two identical columns in both
    scale  one set at 1e3 times the other's scale"""
    rng = np.random.default_rng(zlib.crc32(case_id(kind, n, d).encode()))
    rows = min(n, max(2, d // 2)) if kind == 'short' else n
    x = _gauss(rng, rows, d, 1.0, 0.0)
    y = _gauss(rng, rows, d, 1.7e3 if kind == 'scale' else 1.7, 0.3)
    if kind == 'self':
        y = x.copy()
    elif kind == 'shift':
        y = x + rng.normal(size=d)
    elif kind == 'const':
        x[:, d // 2] = 0.75
        y[:, d // 2] = 0.75
    elif kind == 'twin':
        x[:, d - 1] = x[:, 0]
        y[:, d - 1] = y[:, 0]
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def moments(x):
    """(mean [d], covariance [d, d] over n - 1) of the rows, in float64 from the values as given"""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=0)
    c = x - mu
    return mu, c.T @ c / (x.shape[0] - 1)


def _values(mu1, S1, mu2, S2, tr_sqrt):
    dmu2 = float(np.sum((mu1 - mu2) ** 2))
    tr = float(np.trace(S1) + np.trace(S2))
    return np.array([dmu2 + tr - 2.0 * tr_sqrt, dmu2, tr, 2.0 * tr_sqrt])


def distance(mu1, S1, mu2, S2):
    """[fd, |dmu|^2, tr S1 + tr S2, 2 tr (S1 S2)^(1/2)] by the symmetric square root; not clipped at 0"""
    w, V = np.linalg.eigh(S1)
    r = (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T
    lam = np.linalg.eigvalsh(r @ S2 @ r)
    return _values(mu1, S1, mu2, S2, float(np.sum(np.sqrt(np.clip(lam, 0.0, None)))))


def reference(x, y):
    return distance(*(moments(x) + moments(y)))


def scale_of(v):
    """what an error of the four values is measured against: tr S1 + tr S2 + |dmu|^2"""
    return v[2] + v[1]


def rel_err(got, ref):
    """abs(fd - fd_ref) / (tr S1 + tr S2 + |dmu|^2); two sets of constant equal rows (all of it 0) must give exactly 0"""
    s = scale_of(ref)
    e = abs(float(got[0]) - float(ref[0]))
    return e / s if s > 0 else (0.0 if e == 0 else np.inf)


@functools.lru_cache(None)
def case_model(kind, n, d):
    """model_distance on numpy's float64 moments of a case -> (values, status, sweeps)"""
    x, y = sets(kind, n, d)
    return model_distance(*(moments(x) + moments(y)))


@functools.lru_cache(None)
def case_reference(kind, n, d):
    x, y = sets(kind, n, d)
    v = reference(x, y)
    v.setflags(write=False)
    return v


# ---- the kernel's route ------------------------------------------------------------------------------------------------------------------------
def chol_psd(S):
    """L with L L^T = S for a positive SEMI-definite S, column by column as the kernel: the largest remaining diagonal entry is the pivot (the
    lowest index on a tie), and once it is at or below d eps tr S every remaining column is zero -- never a failure (a constant column,
    n < d, a collapsed generator).  The rows are left in place, so L is lower triangular only up to the pivot order.  Why pivoted: float32
    moments of a rank-deficient set are indefinite at the 1e-8 level, and a factorisation in the given order that takes such a noise
    pivot divides by it -- L L^T then misses S by 1e-4 of its norm; with the largest pivot first it misses by the noise alone."""
    d = S.shape[0]
    thr = max(d * EPS * float(np.trace(S)), 0.0)
    L = np.zeros((d, d))
    dg = np.diag(S).astype(np.float64).copy()
    for j in range(d):
        p = int(np.argmax(dg))                  # (the first of equal values)
        piv = dg[p]
        if not piv > thr:
            break
        live = dg != -np.inf
        col = np.where(live, S[p] - L[:, :j] @ L[p, :j], 0.0) / np.sqrt(piv)
        L[:, j] = col
        dg = np.where(live, dg - col * col, dg)
        dg[p] = -np.inf
    return L


@functools.lru_cache(None)
def round_robin(m, step):
    """the m / 2 disjoint pairs (p < q) of step `step` of a sweep over m columns (m even): m - 1 stays, the others walk a circle"""
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (step + k) % (m - 1)])
    b = np.concatenate([[step], (step - k) % (m - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def rotations(app, aqq, apq):
    """(c, s, t) of the rotations that annihilate a_pq; the identity where a_pq is 0"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        tau = (aqq - app) / (2.0 * apq)
        t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
    t = np.where(apq == 0.0, 0.0, t)
    c = 1.0 / np.sqrt(1.0 + t * t)
    return c, t * c, t


def off_norm(M):
    """the Frobenius norm of the off-diagonal part, summed from those entries alone (||M||^2 - ||diag||^2 cancels at sqrt(eps))"""
    off = M - np.diag(np.diag(M))
    return float(np.sqrt(np.sum(off * off)))


def jacobi_eigenvalues(M, tol=JACOBI_TOL, cap=64):
    """eigenvalues of the symmetric M by two-sided Jacobi rotations in round-robin ordering -> (eigenvalues, sweeps taken, converged).
    The test before every sweep: off(M)_F <= tol ||M at the start||_F."""
    d = M.shape[0]
    m = d + (d & 1)
    A = np.zeros((m, m))
    A[:d, :d] = M
    norm0 = float(np.sqrt(np.sum(A * A)))
    sweeps = 0
    while off_norm(A) > tol * norm0:
        if sweeps == cap:
            return np.diag(A)[:d].copy(), sweeps, False
        for step in range(m - 1):
            p, q = round_robin(m, step)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            c, s, t = rotations(app, aqq, apq)
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = A[q, p] = 0.0
        sweeps += 1
    return np.diag(A)[:d].copy(), sweeps, True


def model_distance(mu1, S1, mu2, S2, cap=64):
    """the kernel's route -> (the four values, status, sweeps)"""
    if not all(np.all(np.isfinite(a)) for a in (mu1, S1, mu2, S2)):
        return np.full(4, np.nan), NONFINITE, 0
    L = chol_psd(S1)
    M = np.tril(L.T @ (S2 @ L))                 # (the kernel forms one triangle and mirrors it)
    lam, sweeps, ok = jacobi_eigenvalues(M + np.tril(M, -1).T, cap=cap)
    tr_sqrt = float(np.sum(np.sqrt(np.clip(lam, 0.0, None))))
    return _values(mu1, S1, mu2, S2, tr_sqrt), (0 if ok else NOT_CONVERGED), sweeps


def fp32_moments(x):
    """what the device's moments may differ by, restated on the host: the fp64 mean, rows centred by it and rounded to float32, a float32
    product summed per block of ROW_BLOCK rows, the block partials in float64 over n - 1"""
    mu = np.asarray(x, np.float64).mean(axis=0)
    c = (np.asarray(x, np.float64) - mu).astype(np.float32)
    S = np.zeros((x.shape[1], x.shape[1]))
    for r0 in range(0, x.shape[0], ROW_BLOCK):
        S += (c[r0:r0 + ROW_BLOCK].T @ c[r0:r0 + ROW_BLOCK]).astype(np.float64)
    return mu, S / (x.shape[0] - 1)
