"""The sliced Wasserstein distance of two sets of projected rows, in float64 numpy, for tests/test_swd_cpu.py and tests/test_swd_gpu.py:
  w_pp(a, b, p)         the yardstick: W_p^p between the empirical measures of the columns of a [m, L] and b [n, L] by the integer-breakpoint
                        formula -- point i of the sorted a owns [i n, (i + 1) n) in units of 1 / (m n), point j of the sorted b owns
                        [j m, (j + 1) m); every interval between two neighbouring breakpoints has one i, one j and an integer length;
  w_pp_lcm(a, b, p)     the brute force for small sizes: every point of a repeated n / g times, every point of b m / g times (g the gcd),
                        then the equal-size formula mean |a_i - b_i|^p;
  reference(px, py, p)  (values, per) as ggan_swd returns them;
  network_sort(keys)    a model of the bitonic network of csrc/swd.hip with its stage order, its two layouts of keys over threads and their
                        index arithmetic, so that those are debugged on the CPU first;
  the grid and the sets the GPU tests run, and their bounds (derived, not measured)."""
import functools
import math
import zlib

import numpy as np

MAX_ROWS, MAX_DIRS, NONFINITE = 16384, 4096, 1        # include/ggan.h: GGAN_SWD_MAX_ROWS, GGAN_SWD_MAX_DIRS, GGAN_SWD_NONFINITE
MIN_PAD, KEYS, SORT_THREADS = 64, 16, 1024            # csrc/swd.hip: kMinPad, kKeys, kSortThreads
EPS = 2.0 ** -52

KINDS = ('gauss', 'shift', 'ties', 'self', 'sorted', 'reversed', 'scale')
EQUAL = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4097, 16384)
UNEQUAL = ((1, 7), (7, 1), (3, 5), (4, 6), (256, 1000), (1000, 999), (512, 1024), (16384, 16383))
SMALL_PAIRS = ((1, 7), (7, 1), (3, 5), (4, 6), (64, 65), (256, 1000), (1000, 999))      # where w_pp_lcm is affordable
DIRS = (1, 3, 64)
PS = (1, 2)


def case_id(kind, m, n, L):
    return '%s-m%d-n%d-L%d' % (kind, m, n, L)


def cases(kinds=KINDS):
    """(kind, m, n, L) over the grid: every equal and unequal size at L = 1, 3 and 64 -- 16384 rows at L = 3 only"""
    sizes = [(n, n) for n in EQUAL] + list(UNEQUAL)
    return [(k, m, n, L) for k in kinds for m, n in sizes for L in DIRS if L == 3 or max(m, n) < 16383]


@functools.lru_cache(None)
def sets(kind, m, n, L):
    """the two float32 sets of projected rows of a case, px [m, L] and py [n, L] (read-only):
    gauss     two Gaussians of unequal scale and mean         self      a set against itself (the same array)
    shift     y = x + c_l per direction, exactly: x and c are multiples of 2^-10 (unequal sizes: rows of x drawn again, then shifted)
    ties      integers 0 .. 3; column 0 is constant 1 in x and 3 in y, the last column constant 2 in both
    sorted    both sets ascending in every column             reversed  both descending
    scale     x at 1e6, y at 1e-6, with +0 and -0 present in both"""
    rng = np.random.default_rng(zlib.crc32(case_id(kind, m, n, L).encode()))
    x = rng.normal(size=(m, L))
    y = 1.7 * rng.normal(size=(n, L)) + 0.3
    if kind == 'self':
        x = x.astype(np.float32)
        x.setflags(write=False)
        return x, x
    if kind == 'shift':
        x = np.round(x * 1024.0) / 1024.0
        c = np.round(rng.normal(size=L) * 1024.0) / 1024.0
        y = (x if m == n else x[rng.integers(0, m, size=n)]) + c
    elif kind == 'ties':
        x, y = rng.integers(0, 4, size=(m, L)).astype(np.float64), rng.integers(0, 4, size=(n, L)).astype(np.float64)
        x[:, L - 1], y[:, L - 1] = 2.0, 2.0
        x[:, 0], y[:, 0] = 1.0, 3.0
    elif kind in ('sorted', 'reversed'):
        x, y = np.sort(x, axis=0), np.sort(y, axis=0)
        if kind == 'reversed':
            x, y = x[::-1], y[::-1]
    elif kind == 'scale':
        x, y = x * 1e6, y * 1e-6
        x[::3, :], y[::4, :] = 0.0, -0.0
        x[1::7, :] = -0.0
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def shift_of(m, n, L):
    """the c_l of the 'shift' case (the draws of sets() again)"""
    rng = np.random.default_rng(zlib.crc32(case_id('shift', m, n, L).encode()))
    rng.normal(size=(m, L))
    rng.normal(size=(n, L))
    return np.round(rng.normal(size=L) * 1024.0) / 1024.0


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def _cols(a):
    a = np.asarray(a, np.float64)
    return a[:, None] if a.ndim == 1 else a


def w_pp(a, b, p):
    """W_p^p per column between the empirical measures of a [m, L] and b [n, L] (or vectors) -> float64 [L].  The breakpoints of the two
    quantile functions are the multiples of n and of m below m n; between two neighbours both are constant."""
    assert p in PS
    a, b = np.sort(_cols(a), axis=0), np.sort(_cols(b), axis=0)
    m, n = a.shape[0], b.shape[0]
    if m == n:
        d = np.ascontiguousarray(np.abs(a - b).T)             # (reduced along the contiguous axis: numpy then sums pairwise)
        return np.mean(d if p == 1 else d * d, axis=1)
    t = np.union1d(np.arange(m, dtype=np.int64) * n, np.arange(n, dtype=np.int64) * m)
    w = np.diff(np.append(t, m * n)).astype(np.float64)
    d = np.ascontiguousarray(np.abs(a[t // n] - b[t // m]).T)
    return np.sum(w * (d if p == 1 else d * d), axis=1) / (float(m) * float(n))


def w_pp_lcm(a, b, p):
    """the same by brute force: both sets repeated to their least common multiple, then the equal-size formula"""
    a, b = np.sort(_cols(a), axis=0), np.sort(_cols(b), axis=0)
    m, n = a.shape[0], b.shape[0]
    g = math.gcd(m, n)
    d = np.ascontiguousarray(np.abs(np.repeat(a, n // g, axis=0) - np.repeat(b, m // g, axis=0)).T)
    return np.mean(d if p == 1 else d * d, axis=1)


def values_of(per, p):
    """[(mean_l per_l)^(1/p), (max_l per_l)^(1/p)], the mean from the exactly rounded sum"""
    mean, mx = math.fsum(per.tolist()) / len(per), float(np.max(per))
    return np.array([mean, mx] if p == 1 else [math.sqrt(mean), math.sqrt(mx)])


def reference(px, py, p):
    """(values float64 [2], per float64 [L]) of float32 (or float64) projected rows"""
    per = w_pp(px, py, p)
    return values_of(per, p), per


@functools.lru_cache(None)
def case_reference(kind, m, n, L, p):
    v, per = reference(*sets(kind, m, n, L), p)
    v.setflags(write=False)
    per.setflags(write=False)
    return v, per


def per_bound(m, n):
    """the relative bound of gate (a) on per: the differences are exact in fp64 and every term is nonnegative, so the fp64 sum of at most
    m + n terms is off by at most that many roundings; four more for the power, the weight, the division and the yardstick's own"""
    return (m + n + 4) * EPS


def values_bound(m, n):
    """... and on values: the same through the mean (nonnegative terms, summed without error) or the max, plus one rounding of the root"""
    return per_bound(m, n) + 0.5 * EPS


# ---- the network of csrc/swd.hip ----------------------------------------------------------------------------------------------------------------
def padded(n):
    p = MIN_PAD
    while p < n:
        p <<= 1
    return p


def layout(P):
    """(KPT, LW) of a padded size, P = 64 KPT << LW: a column below 1024 keys is one wave's, KPT = P / 64 keys a thread; from there on a thread
    holds KEYS keys and 64 << LW threads hold the column"""
    kpt = min(P // 64, KEYS)
    return kpt, (P // (64 * kpt)).bit_length() - 1


def _exchange(lo, hi, up):
    swap = np.where(up, lo > hi, lo < hi)
    return np.where(swap, hi, lo), np.where(swap, lo, hi)


def _keep(v, o, take_min):
    return np.where(take_min, np.where(o < v, o, v), np.where(o > v, o, v))


def _low_stages(S, kpt, lw, k, note):
    """the stages of merge width k with partner distance below 64 KPT, by the 64 << LW threads of the low layout: thread (wave, lane) holds
    the keys i = base | s << 6, base = lane | wave * 64 KPT; distances 32 KPT .. 64 are register s against register s | jb, distances
    32 .. 1 lane against lane ^ j"""
    tid = np.arange(64 << lw)
    lane, base = tid & 63, (tid & 63) | ((tid >> 6) * (64 * kpt))
    v = [S[base | (s << 6)] for s in range(kpt)]
    jb = kpt >> 1
    while jb >= 1:
        if 64 * jb < k:
            for s in range(kpt):
                if not s & jb:
                    v[s], v[s | jb] = _exchange(v[s], v[s | jb], ((base | (s << 6)) & k) == 0)
            note(k, 64 * jb)
        jb >>= 1
    for j in (32, 16, 8, 4, 2, 1):
        if j < k:
            for s in range(kpt):
                v[s] = _keep(v[s], v[s][tid ^ j], (((base | (s << 6)) & k) == 0) == ((lane & j) == 0))
            note(k, j)
    for s in range(kpt):
        S[base | (s << 6)] = v[s]


def _high_stages(S, kpt, lw, k, note):
    """the stages of merge width k with partner distance 64 KPT and above, in the high layout: thread g holds the keys i = g | s * 64 KPT"""
    G, N = 64 * kpt, 1 << lw
    g = np.arange(G)
    u = [S[g + s * G] for s in range(N)]
    jb = N >> 1
    while jb >= 1:
        if G * jb < k:
            for s in range(N):
                if not s & jb:
                    u[s], u[s | jb] = _exchange(u[s], u[s | jb], ((s * G) & k) == 0)
            note(k, G * jb)
        jb >>= 1
    for s in range(N):
        S[g + s * G] = u[s]


def network_sort(keys, trace=None):
    """the kernel's bitonic network on a vector of float32 keys, with its layouts and index arithmetic: padded with +inf to P = padded(n) =
    64 KPT << LW; every merge width up to 64 KPT in the low layout; every wider one a pass in the high layout (distances k / 2 .. 64 KPT),
    then a pass in the low layout.  -> the padded sorted vector.  trace: a list that receives (k, j) of every stage in order."""
    n = len(keys)
    P = padded(n)
    kpt, lw = layout(P)
    S = np.full(P, np.inf, np.float32)
    S[:n] = keys
    note = (lambda k, j: trace.append((k, j))) if trace is not None else (lambda k, j: None)
    k = 2
    while k <= 64 * kpt:
        _low_stages(S, kpt, lw, k, note)
        k <<= 1
    while k <= P:
        _high_stages(S, kpt, lw, k, note)
        _low_stages(S, kpt, lw, k, note)
        k <<= 1
    return S


def network_stages(P):
    """the (k, j) of a bitonic network on P keys, in order: widths 2 .. P, distances k / 2 .. 1 inside each"""
    out, k = [], 2
    while k <= P:
        j = k >> 1
        while j >= 1:
            out.append((k, j))
            j >>= 1
        k <<= 1
    return out
