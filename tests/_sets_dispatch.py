"""Which instance of the set-level Gram-sweep family (csrc/set_rows.h: mmd_sets.hip, knn_sets.hip, knn_lists.hip, parzen_sets.hip and the
assign step of kmeans.hip) each dispatch test runs: one row per kernel instance and edge (plain data), the input recipes of the rows and
their float64 references.

The instances are template arguments picked at run time -- dispatch_k_vec: (K or NS in 1 .. 8) x VEC, dispatch_vec: VEC -- that the names
GGAN_LAUNCH passes do not show.  tests/test_sets_dispatch_gpu.py runs every row through the C entry point it names, asserts that the
profiler saw exactly the row's kernel and the helpers in `also`, once each, with the row's grids, that the GGAN_TRACE_SETS line of the
launch equals `expect`, that every sentinel pad is intact, and that the result matches float64 under the gate the entry already has.
tests/test_sets_dispatch_cpu.py derives every (kernel, K / NS, VEC) the dispatch call sites can produce and fails when one has no row or
a row names one the source no longer produces; it recomputes every `expect`, `also` and workspace size from a Python transcription of the
host code, and checks how little the float64 reference of a row may excuse.

A row:
  kernel   the name GGAN_LAUNCH passes and _lib.prof_report() returns; the instance the name hides is expect['k'], expect['vec']
  entry    mix_rbf_sums | knn_radii | ball_counts | knn_lists | parzen_lse | kmeans_assign (the C entry point, without ggan_)
  shape    (m, n, d): the rows of the first and of the second set and the width; knn_radii: (n, d); kmeans_assign: (rows, centres, d)
  k / ns   knn_radii, knn_lists: k;  mix_rbf_sums, parzen_lse: the number of kernel widths;  else None
  off      the base offset in floats of each input set: 0, or 1 .. 3 for a view into a larger buffer that is not 16-byte aligned
  same     one pointer for both sets;   skip: knn_lists leaves out candidate i for query i
  data     'float' (Gaussian rows, compared under the entry's gate) | 'lattice' (integers 0 .. 3: every distance is exact in float32, the
           result must EQUAL the reference, ties included) | 'count' (kernel widths of 1e6: every kernel value is exactly sum(wts), the
           sums are pair counts in closed form);  seed: of the recipe
  expect   the GGAN_TRACE_SETS line as a dict: k (K, NS, Parzen's run-time ns, 0 where the kernel has none), vec, d, the row counts (m, T
           or nq, nc, c0), the block counts (nb or nbq, nbc), S, grid
  also     the helper launches of the call with their grids in workgroups of 256: the norms pre-pass, the *_final kernel
  note     which edge the row is there for

To add a row: pick the smallest shape that reaches the instance or edge (GGAN_TRACE_SETS=1 prints the choice; plan() of
test_sets_dispatch_cpu.py computes it without a GPU), fill in `expect` and `also`, and run the two dispatch test modules.  If the CPU
module reports that the float64 reference of a knn row leaves too many rows open, change the row's seed.  Float rows stay at a few
hundred rows; a row of thousands is 'lattice' or 'count', so that no float64 distance matrix of that size is ever formed."""
import functools

import numpy as np

import _knn_ref
import _mmd_ref
import _parzen_ref
import _prdc_ref

SIGMAS8 = _mmd_ref.SIGMAS + (3., 7.)                      # a row of ns widths takes the first ns
WTS8 = (0.5, 1.5, 0.75, 2.0, 1.25, 3.0, 0.6, 1.7)         # distinct and none of them 1: a swapped or dropped slot moves the value
COUNT_SIGMAS, COUNT_WTS = (1e6,) * 3, (1., 2., 4.)
MMD_GATE = 2e-5                                           # |v - ref| <= 2e-5 max(1, |ref|), tests/test_mmd_sets_gpu.py
OPEN_ROWS_CAP = 0.05                                      # rows a knn row's reference may leave open (tests/test_knn_gpu.py)
BALL_K = 3                                                # ball_counts rows: the radii are the k-th neighbour distances of the second set


def _xm(k, vec, d, m, T, nb, S, grid):
    return dict(k=k, vec=vec, d=d, m=m, T=T, nb=nb, S=S, grid=grid)


def _xs(k, vec, d, nq, nc, c0, nbq, nbc, S, grid):
    return dict(k=k, vec=vec, d=d, nq=nq, nc=nc, c0=c0, nbq=nbq, nbc=nbc, S=S, grid=grid)


def _row(kernel, entry, shape, expect, also, k=None, ns=None, off=None, same=False, skip=False, data='float', seed=1, note=''):
    off = off if off is not None else ((0,) if entry == 'knn_radii' else (0, 0))
    return dict(kernel=kernel, entry=entry, shape=shape, k=k, ns=ns, off=off, same=same, skip=skip, data=data, seed=seed, expect=expect,
                also=tuple(also), note=note)


def _mmd(shape, ns, expect, norms, **kw):
    return _row('mmd_set_sums', 'mix_rbf_sums', shape, expect, (('mmd_set_norms', norms), ('mmd_set_final', 1)), ns=ns, **kw)


def _radii(shape, k, expect, norms, final=1, **kw):
    return _row('knn_radii', 'knn_radii', shape, expect, (('knn_norms', norms), ('knn_final', final)), k=k, **kw)


def _balls(shape, expect, norms, final=1, **kw):
    return _row('ball_counts', 'ball_counts', shape, expect, (('ball_norms', norms), ('ball_final', final)), **kw)


def _lists(shape, k, expect, norms, final=1, **kw):
    return _row('knn_lists', 'knn_lists', shape, expect, (('knn_lists_norms', norms), ('knn_lists_final', final)), k=k, **kw)


def _parzen(shape, ns, expect, norms, final=1, **kw):
    # every Parzen row is on the lattice, as the small cases of _parzen_ref are: a float32 Gram-form distance is off by up to
    # (2 d + 4) u (|a|^2 + |b|^2) ABSOLUTELY, and lse turns that into err / (2 sigma^2) -- at the narrow bandwidths, where one neighbour
    # decides, that alone exceeds 2e-5 max(1, |ref|) for Gaussian rows (at d = 1, 2 sigma^2 = 0.02 and u (|a|^2 + |b|^2) ~ 6e-7 give 3e-5).
    # On the lattice the distances are exact, so the gate measures the kernel's exp / rescale / log arithmetic and a wrong element shows
    # as a different integer distance.
    kw.setdefault('data', 'lattice')
    return _row('parzen_lse', 'parzen_lse', shape, expect, (('parzen_norms', norms), ('parzen_final', final)), ns=ns, **kw)


def _assign(shape, expect, norms, final=1, **kw):
    return _row('kmeans_assign', 'kmeans_assign', shape, expect,
                (('kmeans_norms', norms), ('kmeans_assign_final', final), ('kmeans_inertia', 1)), **kw)


_LOADERS = ((1, 36), (0, 33))          # (vec, d).  d = 36: two full k-steps and a third with one live quad;  d = 33: the scalar loader
_D_EDGES = ((0, 1), (0, 2), (0, 3), (1, 4), (0, 5), (0, 15), (1, 16), (0, 17), (1, 20))          # (vec, d)
_D1_SEED = 4                           # 130 rows on a line: neighbours left and right tie within float32 in several per cent of the rows;
                                       # this seed leaves none (radii) and one (lists) of them open (test_sets_dispatch_cpu.py asserts it)

ROWS = []

# ---- every instance: K / NS in 1 .. 8 times both loaders; two blocks, a ragged second block, the set boundary inside a tile --------------
ROWS += [_mmd((130, 67, d), ns, _xm(ns, vec, d, 130, 197, 2, 2, (2, 2)), 50, note='NS = %d, %s loader' % (ns, 'float4' if vec else 'scalar'))
         for ns in range(1, 9) for vec, d in _LOADERS]
ROWS += [_radii((130, d), k, _xs(k, vec, d, 130, 130, 0, 2, 2, 2, (2, 2)), 33, note='K = %d, %s loader' % (k, 'float4' if vec else 'scalar'))
         for k in range(1, 9) for vec, d in _LOADERS]
ROWS += [_lists((67, 130, d), k, _xs(k, vec, d, 67, 130, 67, 1, 2, 2, (1, 2)), 50, note='K = %d, %s loader' % (k, 'float4' if vec else 'scalar'))
         for k in range(1, 9) for vec, d in _LOADERS]

# ---- both loaders of the entries without K ------------------------------------------------------------------------------------------------
ROWS += [_balls((130, 67, d), _xs(0, vec, d, 130, 67, 130, 2, 1, 1, (2, 1)), 50) for vec, d in _LOADERS]
ROWS += [_parzen((130, 67, d), ns, _xs(ns, vec, d, 130, 67, 130, 2, 1, 1, (2, 1)), 50, note='ns = %d: %s' % (ns, what))
         for ns, what in ((1, 'the fewest bandwidths'), (16, 'the most')) for vec, d in _LOADERS]
ROWS += [_assign((130, 37, d), _xs(0, vec, d, 130, 37, 130, 2, 1, 1, (2, 1)), 42) for vec, d in _LOADERS]

# ---- the scalar loader chosen by alignment alone: d = 36, one base off a 16-byte boundary; the bits of the aligned call -------------------
ROWS += [
    _mmd((130, 67, 36), 6, _xm(6, 0, 36, 130, 197, 2, 2, (2, 2)), 50, off=(1, 0), note='X off alignment'),
    _mmd((130, 67, 36), 6, _xm(6, 0, 36, 130, 197, 2, 2, (2, 2)), 50, off=(0, 1), note='X aligned, Y not'),
    _radii((130, 36), 3, _xs(3, 0, 36, 130, 130, 0, 2, 2, 2, (2, 2)), 33, off=(1,), note='Z off alignment'),
    _balls((130, 67, 36), _xs(0, 0, 36, 130, 67, 130, 2, 1, 1, (2, 1)), 50, off=(1, 0), note='A off alignment'),
    _balls((130, 67, 36), _xs(0, 0, 36, 130, 67, 130, 2, 1, 1, (2, 1)), 50, off=(0, 3), note='A aligned, B not'),
    _lists((67, 130, 36), 3, _xs(3, 0, 36, 67, 130, 67, 1, 2, 2, (1, 2)), 50, off=(1, 0), note='Q off alignment'),
    _lists((67, 130, 36), 3, _xs(3, 0, 36, 67, 130, 67, 1, 2, 2, (1, 2)), 50, off=(0, 2), note='Q aligned, C not'),
    _parzen((130, 67, 36), 4, _xs(4, 0, 36, 130, 67, 130, 2, 1, 1, (2, 1)), 50, off=(1, 0), note='Q off alignment'),
    _parzen((130, 67, 36), 4, _xs(4, 0, 36, 130, 67, 130, 2, 1, 1, (2, 1)), 50, off=(0, 1), note='Q aligned, S not'),
    _assign((130, 37, 36), _xs(0, 0, 36, 130, 37, 130, 2, 1, 1, (2, 1)), 42, off=(0, 1), note='X aligned, the centres not'),
]

# ---- loader edges in d, one instance per epilogue: below a quad, one quad (the clamp min(k, d - 4) = 0), a ragged last quad ----------------
ROWS += [_mmd((130, 67, d), 6, _xm(6, vec, d, 130, 197, 2, 2, (2, 2)), 50, note='d = %d' % d) for vec, d in _D_EDGES]
ROWS += [_radii((130, d), 3, _xs(3, vec, d, 130, 130, 0, 2, 2, 2, (2, 2)), 33, seed=_D1_SEED if d == 1 else 1, note='d = %d' % d)
         for vec, d in _D_EDGES]
ROWS += [_balls((130, 67, d), _xs(0, vec, d, 130, 67, 130, 2, 1, 1, (2, 1)), 50, note='d = %d' % d) for vec, d in _D_EDGES]
ROWS += [_lists((67, 130, d), 3, _xs(3, vec, d, 67, 130, 67, 1, 2, 2, (1, 2)), 50, seed=_D1_SEED if d == 1 else 1, note='d = %d' % d)
         for vec, d in _D_EDGES]
ROWS += [_parzen((130, 67, d), 4, _xs(4, vec, d, 130, 67, 130, 2, 1, 1, (2, 1)), 50, note='d = %d' % d) for vec, d in _D_EDGES]
ROWS += [_assign((130, 37, d), _xs(0, vec, d, 130, 37, 130, 2, 1, 1, (2, 1)), 42, note='d = %d' % d) for vec, d in _D_EDGES]

# ---- edges in the row counts (d = 20: the quad clamp and the row clamp both act) ----------------------------------------------------------
ROWS += [
    _mmd((128, 67, 20), 6, _xm(6, 1, 20, 128, 195, 2, 2, (2, 2)), 49, note='m = 128: the set boundary on a tile edge'),
    _mmd((128, 128, 20), 6, _xm(6, 1, 20, 128, 256, 2, 2, (2, 2)), 64,
         note='m + n = 256: no ghost row; nb even, S = nt: the first step of workgroup (1, 1) is the half step it does not own'),
    _mmd((129, 127, 20), 6, _xm(6, 1, 20, 129, 256, 2, 2, (2, 2)), 64, note='m + n = 256 with the set boundary one row into a block'),
    _mmd((64, 64, 20), 6, _xm(6, 1, 20, 64, 128, 1, 1, (1, 1)), 32, note='exactly one block: the diagonal tile alone'),
    _mmd((128, 1, 20), 6, _xm(6, 1, 20, 128, 129, 2, 2, (2, 2)), 33, note='129 rows: one real row in the last block, a set of one row'),
    _mmd((130, 130, 36), 6, _xm(6, 1, 36, 130, 260, 3, 2, (3, 2)), 65, same=True, note='same pointer; nb odd'),
    _radii((128, 20), 3, _xs(3, 1, 20, 128, 128, 0, 1, 1, 1, (1, 1)), 32, note='exactly one block'),
    _radii((256, 20), 3, _xs(3, 1, 20, 256, 256, 0, 2, 2, 2, (2, 2)), 64, note='exactly two blocks'),
    _radii((129, 20), 3, _xs(3, 1, 20, 129, 129, 0, 2, 2, 2, (2, 2)), 33, note='one real row in the last block'),
    _radii((9, 20), 8, _xs(8, 1, 20, 9, 9, 0, 1, 1, 1, (1, 1)), 3, note='k = n - 1: every other row is listed'),
    _radii((2, 20), 1, _xs(1, 1, 20, 2, 2, 0, 1, 1, 1, (1, 1)), 1, note='k = n - 1 = 1: a single candidate per row'),
    _balls((128, 128, 20), _xs(0, 1, 20, 128, 128, 128, 1, 1, 1, (1, 1)), 64, note='exactly one block each way'),
    _balls((256, 256, 20), _xs(0, 1, 20, 256, 256, 256, 2, 2, 2, (2, 2)), 128, note='exactly two blocks each way'),
    _balls((129, 129, 20), _xs(0, 1, 20, 129, 129, 129, 2, 2, 2, (2, 2)), 65, note='one real row in the last block, both sides'),
    _balls((130, 1, 20), _xs(0, 1, 20, 130, 1, 130, 2, 1, 1, (2, 1)), 33, note='a single candidate'),
    _lists((128, 128, 20), 3, _xs(3, 1, 20, 128, 128, 128, 1, 1, 1, (1, 1)), 64, note='exactly one block each way'),
    _lists((256, 256, 20), 3, _xs(3, 1, 20, 256, 256, 256, 2, 2, 2, (2, 2)), 128, note='exactly two blocks each way'),
    _lists((129, 129, 20), 3, _xs(3, 1, 20, 129, 129, 129, 2, 2, 2, (2, 2)), 65, note='one real row in the last block, both sides'),
    _lists((130, 1, 20), 1, _xs(1, 1, 20, 130, 1, 130, 2, 1, 1, (2, 1)), 33, note='a single candidate'),
    _lists((67, 5, 20), 5, _xs(5, 1, 20, 67, 5, 67, 1, 1, 1, (1, 1)), 18, note='k = n: every candidate is listed, no ghost row'),
    _lists((9, 9, 20), 8, _xs(8, 1, 20, 9, 9, 9, 1, 1, 1, (1, 1)), 5, skip=True, note='k = n - 1 with skip_diag'),
    _lists((130, 130, 36), 3, _xs(3, 1, 36, 130, 130, 130, 2, 2, 2, (2, 2)), 65, same=True, skip=True,
           note='same pointer, leave-one-out: the diagonal in two tiles'),
    _parzen((128, 128, 20), 4, _xs(4, 1, 20, 128, 128, 128, 1, 1, 1, (1, 1)), 64, note='exactly one block each way'),
    _parzen((256, 256, 20), 4, _xs(4, 1, 20, 256, 256, 256, 2, 2, 2, (2, 2)), 128, note='exactly two blocks each way'),
    _parzen((129, 129, 20), 4, _xs(4, 1, 20, 129, 129, 129, 2, 2, 2, (2, 2)), 65, note='one real row in the last block, both sides'),
    _parzen((130, 1, 20), 4, _xs(4, 1, 20, 130, 1, 130, 2, 1, 1, (2, 1)), 33, note='a single candidate: lse = -D / (2 sigma^2)'),
    _parzen((130, 130, 36), 4, _xs(4, 1, 36, 130, 130, 130, 2, 2, 2, (2, 2)), 65, same=True, note='same pointer: every row meets itself'),
    _assign((128, 128, 20), _xs(0, 1, 20, 128, 128, 128, 1, 1, 1, (1, 1)), 64, note='a full block of rows, a full block of centres'),
    _assign((256, 37, 20), _xs(0, 1, 20, 256, 37, 256, 2, 1, 1, (2, 1)), 74, note='exactly two blocks of rows'),
    _assign((129, 1, 20), _xs(0, 1, 20, 129, 1, 129, 2, 1, 1, (2, 1)), 33, note='one real row in the last block; a single centre'),
]

# ---- splits: a workgroup walks more than one tile.  Thousands of rows: exact data, references in closed form or from integer Gram blocks --
ROWS += [
    _mmd((4100, 4000, 16), 3, _xm(3, 1, 16, 4100, 8100, 64, 32, (64, 32)), 2025, data='count',
         note='64 blocks, 33 steps in 32 splits: split 0 walks two steps, and its second, the half step, is skipped for a >= 32'),
    _mmd((2900, 2900, 16), 3, _xm(3, 1, 16, 2900, 5800, 46, 24, (46, 24)), 1450, data='count',
         note='46 blocks, S = nt = 24: the FIRST step of split 23 is the half step, invalid for a >= 23 -- such a workgroup leaves zeros'),
    _radii((5800, 16), 3, _xs(3, 1, 16, 5800, 5800, 0, 46, 46, 45, (46, 45)), 1450, final=23, data='lattice',
           note='46 candidate blocks in 45 splits: split 0 walks a second, ragged tile'),
    _balls((5800, 5800, 16), _xs(0, 1, 16, 5800, 5800, 5800, 46, 46, 45, (46, 45)), 2900, final=23, data='lattice',
           note='46 candidate blocks in 45 splits'),
    _lists((5800, 5800, 16), 3, _xs(3, 1, 16, 5800, 5800, 5800, 46, 46, 45, (46, 45)), 2900, final=23, data='lattice',
           note='46 candidate blocks in 45 splits'),
    _parzen((5800, 5800, 16), 4, _xs(4, 1, 16, 5800, 5800, 5800, 46, 46, 45, (46, 45)), 2900, final=23, data='lattice',
            note='46 candidate blocks in 45 splits: the shifted sums of two tiles and 45 partials are rescaled and combined'),
]


def instance(row):
    """the (kernel, K / NS or None, VEC) triple of the template instance a row runs"""
    templ = row['entry'] in ('mix_rbf_sums', 'knn_radii', 'knn_lists')
    return row['kernel'], (row['expect']['k'] if templ else None), bool(row['expect']['vec'])


def row_id(row):
    x = row['expect']
    return '%s-k%d-vec%d-%s%s%s%s%s' % (row['kernel'], x['k'], x['vec'], 'x'.join(str(v) for v in row['shape']),
                                        '-off%s' % ''.join(str(v) for v in row['off']) if any(row['off']) else '', '-same' if row['same'] else '',
                                        '-skip' if row['skip'] else '', '' if row['data'] == 'float' else '-' + row['data'])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def dims(row):
    """(m, n, d) with n = m for the one-set entry"""
    s = row['shape']
    return (s[0], s[0], s[1]) if row['entry'] == 'knn_radii' else s


@functools.lru_cache(maxsize=None)
def _sets(data, seed, m, n, d, same):
    rng = np.random.default_rng(100003 * seed + 1000 * m + 10 * n + d)
    if data == 'lattice':
        A, B = rng.integers(0, 4, size=(m, d)).astype(np.float32), rng.integers(0, 4, size=(n, d)).astype(np.float32)
    else:
        A, B = (rng.standard_normal((m, d)) * 1.5).astype(np.float32), (rng.standard_normal((n, d)) + 0.3).astype(np.float32)
    if same:
        B = A
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def sets(row):
    """(A [m, d], B [n, d]) float32, read-only, made once per run; knn_radii uses A alone; same: B is A"""
    m, n, d = dims(row)
    return _sets(row['data'], row['seed'], m, n, d, row['same'])


def mmd_widths(row):
    if row['data'] == 'count':
        return COUNT_SIGMAS, COUNT_WTS
    return SIGMAS8[:row['ns']], WTS8[:row['ns']]


def parzen_widths(row):
    """ns bandwidths from nearest-neighbour-only up to every-candidate-counts, as _parzen_ref.LATTICE_FACTORS times sqrt(4 d)"""
    d = row['shape'][2]
    lo, hi = _parzen_ref.LATTICE_FACTORS[0], _parzen_ref.LATTICE_FACTORS[-1]
    return np.geomspace(lo, hi, row['ns']) * np.sqrt(4.0 * d) if row['ns'] > 1 else np.array([np.sqrt(4.0 * d)])


# ---- float64 references, cached per shape and recipe (rows that differ in K, NS or the base offset share them) ------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _d2(data, seed, m, n, d, same, which):
    """float64 squared distances from direct differences: 'ab' [m, n], 'aa' [m, m], 'bb' [n, n]"""
    A, B = _sets(data, seed, m, n, d, same)
    X, Y = dict(ab=(A, B), aa=(A, A), bb=(B, B))[which]
    return _frozen(_prdc_ref.d2(X, Y))[0]


def d2(row, which='ab'):
    m, n, d = dims(row)
    assert row['data'] == 'float' and max(m, n) <= 1024, 'a float64 distance matrix is for the small float rows'
    return _d2(row['data'], row['seed'], m, n, d, row['same'], which)


@functools.lru_cache(maxsize=None)
def _mmd_sums(seed, m, n, d, same, ns):
    A, B = _sets('float', seed, m, n, d, same)
    return _frozen(_mmd_ref.sums3(A, B, SIGMAS8[:ns], WTS8[:ns]))[0]


def mmd_reference(row):
    """[S_xx, S_yy, S_xy] in float64; 'count' rows: the pair counts times sum(wts)"""
    m, n, d = row['shape']
    if row['data'] == 'count':
        w = float(sum(COUNT_WTS))
        return np.array([w * m * (m - 1), w * n * (n - 1), w * m * n])
    return _mmd_sums(row['seed'], m, n, d, row['same'], row['ns'])


def knn_reference(row):
    """_knn_ref.closed_rows of a float knn_radii / knn_lists row (+ D, T): radii are leave-one-out lists of a set against itself"""
    A, B = sets(row)
    if row['entry'] == 'knn_radii':
        D, T = np.array(d2(row, 'aa')), _knn_ref.row_tol(A, A)
        np.fill_diagonal(D, np.inf)
    else:
        D, T = np.array(d2(row, 'ab')), _knn_ref.row_tol(A, B)
        if row['skip']:
            np.fill_diagonal(D, np.inf)
    out = _knn_ref.closed_rows(D, row['k'], T)
    out.update(D=D, T=T)
    return out


def ball_radii(row):
    """the squared radii of a ball_counts row, float64: the BALL_K-th neighbour distance within the second set; a set too small for that
    (and the lattice rows): the median distance of each candidate to the queries, an integer on the lattice"""
    A, B = sets(row)
    if row['data'] == 'lattice':
        rng = np.random.default_rng(row['seed'])
        return rng.integers(2 * B.shape[1], 3 * B.shape[1], size=B.shape[0]).astype(np.float64)      # around the mean distance 2.5 d
    if B.shape[0] > BALL_K:
        return _prdc_ref.radii_from(d2(row, 'bb'), BALL_K)
    return np.median(d2(row, 'ab'), axis=0)


def lattice_blocks(A, B, step=512):
    """(r0, D) over blocks of `step` rows of A: the squared distances [rows, n] as exact integers in float64, from the Gram form (every
    product and sum is an integer far below 2^53) -- no matrix of size m n is held"""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    nb = (B64 * B64).sum(1)
    for r0 in range(0, A64.shape[0], step):
        a = A64[r0:r0 + step]
        yield r0, (a * a).sum(1)[:, None] + nb[None, :] - 2.0 * (a @ B64.T)


def lattice_lists(A, B, k, skip):
    """(idx [m, k], dist [m, k]) of a lattice row, ascending in (distance, index), from integer keys distance * 2^17 + index"""
    idx, dist = [], []
    for r0, D in lattice_blocks(A, B):
        key = D.astype(np.int64) * (1 << 17) + np.arange(B.shape[0], dtype=np.int64)[None, :]
        if skip:
            rows = np.arange(D.shape[0])
            key[rows, r0 + rows] = np.iinfo(np.int64).max
        best = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
        idx.append(best & ((1 << 17) - 1))
        dist.append((best >> 17).astype(np.float64))
    return np.concatenate(idx), np.concatenate(dist)
