"""float64 numpy restatement of tflib/objs/mmd.py:20-67 for the tests: the three pairwise mixture-of-RBF sums from DIRECT differences (not
the Gram form the kernels use), and both MMD^2 estimators from those sums."""
import numpy as np

SIGMAS = (2., 5., 10., 20., 40., 80.)


def _kernel(A, B, sigmas, wts):
    """K[i, j] = sum_s wt_s exp(-||a_i - b_j||^2 / (2 sigma_s^2)), rows of A in chunks (the [rows, rows, d] difference is never whole)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    K = np.zeros((A.shape[0], B.shape[0]))
    step = max(1, int(4e6 // max(1, B.shape[0] * A.shape[1])))
    for r0 in range(0, A.shape[0], step):
        D = ((A[r0:r0 + step, None, :] - B[None, :, :]) ** 2).sum(-1)
        for sg, wt in zip(sigmas, wts):
            K[r0:r0 + step] += wt * np.exp(-D / (2.0 * sg * sg))
    return K


def sums3(X, Y, sigmas=SIGMAS, wts=None):
    """[S_xx, S_yy, S_xy]: the same-set sums over ordered pairs i != j, the cross sum over every pair"""
    wts = [1.0] * len(sigmas) if wts is None else [float(w) for w in wts]
    Kxx, Kyy, Kxy = _kernel(X, X, sigmas, wts), _kernel(Y, Y, sigmas, wts), _kernel(X, Y, sigmas, wts)
    return np.array([Kxx.sum() - np.trace(Kxx), Kyy.sum() - np.trace(Kyy), Kxy.sum()])


def from_sums(s3, m, n, wt_sum, biased):
    """the reference's diagonal is the constant sum(wts) (mmd.py:52-54,67)"""
    sxx, syy, sxy = (float(v) for v in s3)
    if biased:
        return (sxx + m * wt_sum) / (m * m) + (syy + n * wt_sum) / (n * n) - 2.0 * sxy / (m * n)
    return sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - 2.0 * sxy / (m * n)


def mmd2(X, Y, sigmas=SIGMAS, wts=None, biased=True):
    wt_sum = float(len(sigmas)) if wts is None else float(sum(wts))
    return from_sums(sums3(X, Y, sigmas, wts), len(X), len(Y), wt_sum, biased)


def mmd2_direct(X, Y, sigmas=SIGMAS, wts=None, biased=True):
    """_mmd2 (mmd.py:43-63) written out on the full kernel matrices, diagonals included: what from_sums must reproduce"""
    w = [1.0] * len(sigmas) if wts is None else [float(v) for v in wts]
    Kxx, Kyy, Kxy = _kernel(X, X, sigmas, w), _kernel(Y, Y, sigmas, w), _kernel(X, Y, sigmas, w)
    m, n = float(len(X)), float(len(Y))
    if biased:
        return Kxx.sum() / (m * m) + Kyy.sum() / (n * n) - 2.0 * Kxy.sum() / (m * n)
    return (Kxx.sum() - np.trace(Kxx)) / (m * (m - 1)) + (Kyy.sum() - np.trace(Kyy)) / (n * (n - 1)) - 2.0 * Kxy.sum() / (m * n)
