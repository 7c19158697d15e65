"""The coverage table tests/_sets_dispatch.py against the set-level Gram-sweep family (csrc/set_rows.h and the .hip files built on it):
every (kernel, K / NS, VEC) instance the dispatch_vec / dispatch_k_vec call sites can produce has a row, and no row names one the source
no longer produces; every row's `expect`, `also` and workspace size follow from a Python transcription of the host code (blocks_of,
splits_of, mmd_splits_of, step_valid, the vec predicate, the grids, the partial layouts); the transcribed walks cover every block pair /
candidate block exactly once at every block count that matters; and the float64 reference of a row excuses little.  Reads the project's
own source for names and constants only."""
import glob
import os
import re

import numpy as np
import pytest

import _mmd_ref
import _sets_dispatch as D
from _sets_dispatch import ROWS, row_id

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graphical_gan_amd', 'csrc')
SWEEPS = ('knn_radii', 'ball_counts', 'knn_lists', 'parzen_lse', 'kmeans_assign')
BLOCK_COUNTS = list(range(1, 65)) + [127, 128, 129, 2047, 2048]          # 2048 = 2 x 131072 / 128


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- instances against rows ------------------------------------------------------------------------------------------------------------------
def _call_body(text, start):
    """the text of the call whose opening parenthesis is at text[start], up to its matching close"""
    depth = 0
    for i in range(start, len(text)):
        depth += text[i] == '('
        depth -= text[i] == ')'
        if depth == 0:
            return text[start:i + 1]
    raise AssertionError('unbalanced call')


_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"')


def k_range(header):
    """(first, last) K of dispatch_k_vec, from its default template argument and its `if constexpr (K > last)`"""
    m = re.search(r'template <int K = (\d+), class F>\s*inline int dispatch_k_vec\(.*?if constexpr \(K > (\d+)\)', header, flags=re.S)
    assert m, 'dispatch_k_vec not found'
    return int(m.group(1)), int(m.group(2))


def source_instances(files, header):
    """-> ({(name, K or None, VEC)}, {helper names launched inside a dispatch call without VEC})"""
    k0, k1 = k_range(header)
    out, helpers = set(), set()
    for text in files:
        for m in re.finditer(r'\b(dispatch_k_vec|dispatch_vec)\(', text):
            body = _call_body(text, m.end() - 1)
            for lm in _LAUNCH.finditer(body):
                launch = _call_body(body, body.index('(', lm.start()))
                if 'decltype(VEC)::value' not in launch:
                    helpers.add(lm.group(1))
                    continue
                ks = range(k0, k1 + 1) if m.group(1) == 'dispatch_k_vec' else (None,)
                out |= {(lm.group(1), k, v) for k in ks for v in (False, True)}
    return out, helpers


def _sources():
    return [open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.hip')))], _read('set_rows.h')


def uncovered(files, header, rows=ROWS):
    src, _ = source_instances(files, header)
    have = {D.instance(r) for r in rows}
    key = lambda t: (t[0], -1 if t[1] is None else t[1], t[2])
    return sorted(src - have, key=key), sorted(have - src, key=key)


def test_parser_reads_both_dispatchers_and_the_range():
    header = 'template <int K = 2, class F>\ninline int dispatch_k_vec(int k, bool vec, F&& f) {\n    if constexpr (K > 3) {\n'
    text = ('    return dispatch_k_vec(k, P.vec, [&](auto K, auto VEC) {\n        constexpr int kk = decltype(K)::value;\n'
            '        GGAN_LAUNCH("a", L.flops, f(x), (a_k<kk, decltype(VEC)::value>), L.grid, dim3(256), 0, st, P);\n'
            '        GGAN_LAUNCH("a_final", 0, 4.0 * n, a_final_k<kk>, dim3(cdiv(n, 256)), dim3(256), 0, st, n);\n        return 0;\n    });\n'
            '    if (const int rc = dispatch_vec(P.vec, [&](auto VEC) {\n'
            '            GGAN_LAUNCH("b", 0, 0, b_k<decltype(VEC)::value>, L.grid, dim3(256), 0, st, P);\n            return 0;\n        }))\n')
    src, helpers = source_instances([text], header)
    assert src == {('a', 2, False), ('a', 2, True), ('a', 3, False), ('a', 3, True), ('b', None, False), ('b', None, True)}
    assert helpers == {'a_final'}


def test_every_instance_has_a_row_and_every_row_an_instance():
    files, header = _sources()
    src, helpers = source_instances(files, header)
    assert k_range(header) == (1, 8)
    assert {t[0] for t in src} == {'mmd_set_sums'} | set(SWEEPS), sorted({t[0] for t in src})
    assert len(src) == 3 * 16 + 3 * 2
    missing, stale = uncovered(files, header)
    assert not missing, 'instances without a row in tests/_sets_dispatch.py: %s' % missing
    assert not stale, 'rows for instances the source no longer produces: %s' % stale
    # the helpers a dispatch call launches beside its instance are in the rows' `also`
    assert helpers <= {a for r in ROWS for a, _ in r['also']}, helpers


def test_a_deleted_row_and_a_widened_range_are_noticed():
    files, header = _sources()
    victim = ('knn_lists', 7, False)
    rows = [r for r in ROWS if D.instance(r) != victim]
    assert len(rows) < len(ROWS) and uncovered(files, header, rows) == ([victim], [])
    wider = header.replace('if constexpr (K > 8)', 'if constexpr (K > 9)')
    assert wider != header
    missing, stale = uncovered(files, header=wider)
    assert sorted(missing) == sorted((n, 9, v) for n in ('mmd_set_sums', 'knn_radii', 'knn_lists') for v in (False, True)) and not stale
    narrower = header.replace('if constexpr (K > 8)', 'if constexpr (K > 7)')
    assert len(uncovered(files, header=narrower)[1]) == 6


def test_the_table_keeps_the_cases_it_was_written_for():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    by = lambda entry: [r for r in ROWS if r['entry'] == entry]
    for entry in ('mix_rbf_sums', 'knn_radii', 'ball_counts', 'knn_lists', 'parzen_lse', 'kmeans_assign'):
        rows = by(entry)
        # both loaders; the scalar loader by alignment alone; the widths around a quad; 128, 129 and 256 rows
        assert {r['expect']['vec'] for r in rows} == {0, 1}
        assert any(r['expect']['vec'] == 0 and r['shape'][-1] % 4 == 0 and any(r['off']) for r in rows), entry
        assert {r['shape'][-1] for r in rows} >= {1, 2, 3, 4, 5, 15, 16, 17, 20, 33, 36}, entry
        assert {r['expect']['T'] if entry == 'mix_rbf_sums' else r['shape'][0] for r in rows} >= {128, 129, 256}, entry
    for entry in ('mix_rbf_sums', 'ball_counts', 'knn_lists', 'parzen_lse'):
        offs = {r['off'] for r in by(entry) if any(r['off'])}
        assert any(o[0] and not o[1] for o in offs) and any(o[1] and not o[0] for o in offs), (entry, offs)
    for entry in ('mix_rbf_sums', 'knn_lists', 'parzen_lse'):
        assert any(r['same'] for r in by(entry)), entry
    for entry in ('ball_counts', 'knn_lists', 'parzen_lse'):
        assert any(r['expect']['nc'] == 1 for r in by(entry)), entry
    assert {r['ns'] for r in by('parzen_lse')} >= {1, 16}
    assert any(r['k'] == r['shape'][0] - 1 for r in by('knn_radii'))
    assert any(r['k'] == r['shape'][1] and not r['skip'] for r in by('knn_lists'))
    assert any(r['k'] == r['shape'][1] - 1 and r['skip'] for r in by('knn_lists'))
    assert any(r['shape'][0] == 128 for r in by('mix_rbf_sums')) and any(sum(r['shape'][:2]) == 256 for r in by('mix_rbf_sums'))
    # splits: a workgroup that walks two tiles, the last of them ragged
    for entry in SWEEPS[:-1]:
        assert any(r['expect']['nbc'] % r['expect']['S'] and r['expect']['nbc'] > r['expect']['S'] and r['expect']['nc'] % 128 for r in by(entry))
    big = [r for r in ROWS if max(r['shape'][:-1]) > 1024]
    assert big and all(r['data'] in ('lattice', 'count') for r in big)


# ---- the transcription -----------------------------------------------------------------------------------------------------------------------
def _const(header, name):
    return int(re.search(r'constexpr int %s = (\d+);' % name, header).group(1))


BT, TARGET, MAX_ROWS = (_const(_read('set_rows.h'), n) for n in ('BT', 'kTargetWgs', 'kMaxRows'))
ROW_BLOCK = 512                                                   # GGAN_KMEANS_ROW_BLOCK (tests/_kmeans_ref.py holds it too)


def cdiv(a, b):
    return (a + b - 1) // b


def align16(b):
    return (b + 15) & ~15


def norms_bytes(rows):
    return align16(4 * rows)


def blocks_of(rows):
    return cdiv(rows, BT)


def splits_of(nbq, nbc):
    return max(1, min(cdiv(TARGET, nbq), nbc))


def mmd_splits_of(nb):
    return max(1, min(cdiv(TARGET, nb), nb // 2 + 1))


def step_valid(a, t, nb):
    return 2 * t < nb or (2 * t == nb and 2 * a < nb) or t == 0


def vec_of(d, offs):
    """float4 loads are legal: d % 4 == 0 and every base 16-byte aligned (the buffers themselves are)"""
    return int(d % 4 == 0 and all((4 * o) % 16 == 0 for o in offs))


def plan(row):
    """-> (expect, also, workspace bytes) of a row from its shape, k / ns and base offsets alone"""
    entry, off = row['entry'], row['off']
    m, n, d = D.dims(row)
    vec = vec_of(d, off)
    if entry == 'mix_rbf_sums':
        T = m + n
        nb = blocks_of(T)
        S = mmd_splits_of(nb)
        return (dict(k=row['ns'], vec=vec, d=d, m=m, T=T, nb=nb, S=S, grid=(nb, S)),
                (('mmd_set_norms', cdiv(T, 4)), ('mmd_set_final', 1)), norms_bytes(T) + nb * S * 3 * 8)
    if entry == 'knn_radii':
        nq, nc, c0, T = m, m, 0, m
    else:
        nq, nc, c0, T = m, n, m, m + n
    nbq, nbc = blocks_of(nq), blocks_of(nc)
    S = 1 if entry == 'kmeans_assign' else splits_of(nbq, nbc)
    k = dict(knn_radii=row['k'], knn_lists=row['k'], parzen_lse=row['ns']).get(entry, 0)
    x = dict(k=k, vec=vec, d=d, nq=nq, nc=nc, c0=c0, nbq=nbq, nbc=nbc, S=S, grid=(nbq, S))
    final = cdiv(nq, 256)
    if entry == 'knn_radii':
        return x, (('knn_norms', cdiv(T, 4)), ('knn_final', final)), norms_bytes(T) + S * k * nq * 4
    if entry == 'ball_counts':                                    # two planes [S][nq], minima and counts, each rounded to 16 bytes
        return x, (('ball_norms', cdiv(T, 4)), ('ball_final', final)), norms_bytes(T) + 2 * align16(S * nq * 4)
    if entry == 'knn_lists':
        return x, (('knn_lists_norms', cdiv(T, 4)), ('knn_lists_final', final)), norms_bytes(T) + S * k * nq * 8
    if entry == 'parzen_lse':
        return x, (('parzen_norms', cdiv(T, 4)), ('parzen_final', final)), norms_bytes(T) + S * (1 + k) * nq * 4
    assert entry == 'kmeans_assign' and nbc == 1
    ub = cdiv(nq, ROW_BLOCK)
    ws = norms_bytes(T) + align16(8 * nq) + 2 * align16(4 * nq) + align16(4 * ub * nc * d) + align16(4 * ub * nc)
    return x, (('kmeans_norms', cdiv(T, 4)), ('kmeans_assign_final', final), ('kmeans_inertia', 1)), ws


def workspace_of(L, row):
    m, n, d = D.dims(row)
    e = row['entry']
    return (L.ggan_mix_rbf_sums_workspace(m, n) if e == 'mix_rbf_sums' else L.ggan_knn_radii_workspace(m, row['k']) if e == 'knn_radii' else
            L.ggan_ball_counts_workspace(m, n) if e == 'ball_counts' else L.ggan_knn_lists_workspace(m, n, row['k']) if e == 'knn_lists' else
            L.ggan_parzen_lse_workspace(m, n, row['ns']) if e == 'parzen_lse' else L.ggan_kmeans_workspace(m, d, n))


def test_the_transcription_reads_the_constants_it_restates():
    header, mmd, kmeans = _read('set_rows.h'), _read('mmd_sets.hip'), _read('kmeans.hip')
    assert (BT, TARGET, MAX_ROWS) == (128, 2048, 131072)
    for text, what in ((header, 'return (int)((rows + BT - 1) / BT);'), (header, 'int S = (kTargetWgs + nbq - 1) / nbq;'),
                       (header, 'if (S > nbc) S = nbc;'), (mmd, 'int S = (kTargetWgs + nb - 1) / nb;'), (mmd, 'if (S > nt) S = nt;'),
                       (mmd, 'return 2 * t < nb || (2 * t == nb && 2 * a < nb) || t == 0;'),
                       (header, 'P.vec = (d % 4 == 0) && ((uintptr_t)P.X & 15) == 0 && ((uintptr_t)P.Y & 15) == 0;'),
                       (kmeans, 'R.vec = (d % 4 == 0) && ((uintptr_t)R.X & 15) == 0 && ((uintptr_t)R.Y & 15) == 0;'),
                       (kmeans, 'P.nbc = 1; P.S = 1;')):
        assert what in text, what
    assert re.search(r'#define GGAN_KMEANS_ROW_BLOCK\s+%d\b' % ROW_BLOCK, open(os.path.join(CSRC, '..', '..', 'include', 'ggan.h')).read())


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_expect_follows_from_the_transcription(idx):
    row = ROWS[idx]
    x, also, _ = plan(row)
    assert row['expect'] == x, (row['expect'], x)
    assert row['also'] == also, (row['also'], also)
    m, n, d = D.dims(row)
    assert 1 <= m <= MAX_ROWS and 1 <= n <= MAX_ROWS and d >= 1 and len(row['off']) == (1 if row['entry'] == 'knn_radii' else 2)
    assert all(0 <= o <= 3 for o in row['off']) and (not row['same'] or (m == n and row['off'][0] == row['off'][1]))
    if row['entry'] in ('knn_radii', 'knn_lists'):
        assert 1 <= row['k'] <= n - (1 if row['skip'] or row['entry'] == 'knn_radii' else 0)
    assert not row['skip'] or (row['entry'] == 'knn_lists' and m == n)


def test_workspace_entries_agree_with_the_partial_layouts(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    for row in ROWS:
        assert workspace_of(L, row) == plan(row)[2], (row_id(row), workspace_of(L, row), plan(row)[2])


# ---- block coverage, from the transcription alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', BLOCK_COUNTS)
def test_the_symmetric_walk_visits_every_unordered_block_pair_once(nb):
    S, nt = mmd_splits_of(nb), nb // 2 + 1
    a, s = np.meshgrid(np.arange(nb), np.arange(S), indexing='ij')
    seen = np.zeros((nb, nb), np.int64)
    tiles = np.zeros((nb, S), np.int64)
    for j in range(cdiv(nt, S)):                                  # workgroup (a, s) walks t = s, s + S, ... as far as they are tiles
        t = s + j * S
        ok = (t < nt) & ((2 * t < nb) | ((2 * t == nb) & (2 * a < nb)) | (t == 0))
        b = (a + t) % nb
        lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
        np.add.at(seen, (lo, hi), 1)
        tiles += ok
    assert np.array_equal(seen, np.triu(np.ones((nb, nb), np.int64))), 'a block pair is missed or visited twice'
    assert int(tiles.sum()) == nb * (nb + 1) // 2
    assert 1 <= S <= nt and nb * S <= max(TARGET + nb, nb)
    # the vectorised condition above is step_valid
    for aa, tt in ((0, 0), (nb - 1, nb // 2), (0, nb // 2), (nb // 2, nb // 2), (nb - 1, 0)):
        assert bool((2 * tt < nb) or (2 * tt == nb and 2 * aa < nb) or tt == 0) == step_valid(aa, tt, nb)
    # every workgroup of the grid (nb, S) writes its triple, tiles or none: the last stage adds all nb * S of them, and the workspace
    # holds exactly that many
    assert norms_bytes(nb * BT) + nb * S * 24 == plan(dict(entry='mix_rbf_sums', shape=(nb * BT - 1, 1, 4), off=(0, 0), ns=1))[2]
    if nb % 2 == 0 and S == nt:                                  # then some workgroups have no tile at all: their partial is the zeros
        assert int((tiles == 0).sum()) == nb // 2
    else:
        assert int((tiles == 0).sum()) == 0


@pytest.mark.parametrize('nbc', BLOCK_COUNTS)
def test_every_candidate_block_falls_in_exactly_one_split(nbc):
    for nbq in sorted({1, 2, 3, 45, 46, 47, 1024, 1025, nbc}):
        S = splits_of(nbq, nbc)
        assert 1 <= S <= nbc
        seen = np.zeros(nbc, np.int64)
        for s in range(S):
            seen[s::S] += 1                                       # c = s, s + S, ... < nbc
        assert np.all(seen == 1), (nbq, nbc, S)
        assert nbq * S <= TARGET + nbq or S == 1


# ---- how little a row's reference may excuse ----------------------------------------------------------------------------------------------
KNN_ROWS = [i for i, r in enumerate(ROWS) if r['entry'] in ('knn_radii', 'knn_lists')]


@pytest.mark.parametrize('idx', KNN_ROWS, ids=[row_id(ROWS[i]) for i in KNN_ROWS])
def test_closed_rows_can_hide_little(idx):
    """the GPU test holds a row of a list to the reference only where float32 cannot decide differently: at most 5 % of the rows may be
    left open by the reference's own tie bands, and at least one row must be pinned position by position.  Lattice rows excuse nothing:
    they are compared exactly, ties included."""
    row = ROWS[idx]
    if row['data'] == 'lattice':
        A, B = D.sets(row)
        assert np.array_equal(A, np.round(A)) and A.min() >= 0 and A.max() <= 3 and B.min() >= 0 and B.max() <= 3
        assert A.shape[1] * 9 * (1 << 17) < 2 ** 53 and B.shape[0] < (1 << 17)          # lattice_lists' integer keys
        return
    r = D.knn_reference(row)
    open_ = float(np.mean(~r['set_closed']))
    print('%s: open rows %.4f, pinned positions %d of %d' % (row_id(row), open_, int(r['pinned'].sum()), r['pinned'].size))
    assert open_ <= D.OPEN_ROWS_CAP, (row_id(row), open_)
    assert r['pinned'].any(), row_id(row)


def test_kmeans_rows_leave_few_rows_ambiguous():
    import _kmeans_ref as K
    for row in ROWS:
        if row['entry'] == 'kmeans_assign':
            X, C = D.sets(row)
            amb = K.ambiguous(D.d2(row), K.tol(X, C).max(axis=1))
            assert amb.mean() <= K.AMBIGUOUS_CAP, (row_id(row), amb.mean())


def test_a_swapped_or_dropped_width_moves_the_mmd_beyond_the_gate():
    """the NS rows carry distinct widths and distinct weights: leaving out slot s, or exchanging the weights (or the widths) of slots i and
    j, moves both estimators by more than the gate, so an instance that reads a wrong g2 / wt register cannot pass"""
    seen = 0
    for row in ROWS:
        if row['entry'] != 'mix_rbf_sums' or row['data'] != 'float' or row['shape'][:2] != (130, 67) or row['shape'][2] not in (33, 36):
            continue
        m, n, d = row['shape']
        X, Y = D.sets(row)
        ns = row['ns']
        sig, wts = D.mmd_widths(row)
        assert len(sig) == len(wts) == ns and len(set(sig)) == ns and len(set(wts)) == ns and 1.0 not in wts
        per = [_mmd_ref.sums3(X, Y, (s,), (1.0,)) for s in sig]
        for biased in (True, False):
            one = [_mmd_ref.from_sums(p, m, n, 1.0, biased) for p in per]
            ref = sum(w * v for w, v in zip(wts, one))
            assert abs(ref - _mmd_ref.from_sums(D.mmd_reference(row), m, n, float(sum(wts)), biased)) < 1e-12
            gate = D.MMD_GATE * max(1.0, abs(ref))
            for i in range(ns):
                assert abs(wts[i] * one[i]) > 2 * gate, ('dropped', ns, i, wts[i] * one[i], gate)
                for j in range(i):
                    assert abs((wts[i] - wts[j]) * (one[i] - one[j])) > 2 * gate, ('swapped', ns, i, j, gate)
        seen += 1
    assert seen >= 16


# ---- the GPU module's checks have teeth: a float32 Gram-form emulation passes them, the neighbouring wrong instance does not ---------------
def _gram32(A, B):
    """squared distances as the kernels form them, in float32: max(n_i + n_j - 2 a.b, 0)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    na, nb = (A * A).sum(1, dtype=np.float32), (B * B).sum(1, dtype=np.float32)
    return np.maximum(na[:, None] + nb[None, :] - np.float32(2) * (A @ B.T), np.float32(0))


def _first(entry, **want):
    return next(r for r in ROWS if r['entry'] == entry and r['data'] == 'float' and all(r[k] == v for k, v in want.items()))


def test_the_gpu_checks_reject_the_neighbouring_instance():
    import test_sets_dispatch_gpu as G
    # radii: the K-th distance passes, the (K - 1)-th -- a list one register short -- misses the bound
    row = _first('knn_radii', k=3, shape=(130, 36))
    A, _ = D.sets(row)
    Dg = _gram32(A, A)
    np.fill_diagonal(Dg, np.inf)
    srt = np.sort(Dg, axis=1)
    assert G._radii_fractions(row, dict(r2=srt[:, 2].copy()))['radii'] <= 1.0
    assert G._radii_fractions(row, dict(r2=srt[:, 1].copy()))['radii'] > 1.0
    # lists: the emulated lists pass; two neighbouring positions exchanged in one pinned row do not
    row = _first('knn_lists', k=5, shape=(67, 130, 36))
    A, B = D.sets(row)
    Dg = _gram32(A, B)
    idx = np.argsort(Dg, axis=1, kind='stable')[:, :5].astype(np.int32)
    d2 = np.take_along_axis(Dg, idx.astype(np.int64), axis=1)
    assert G._lists_fractions(row, dict(idx=idx, d2=d2))['lists'] <= 1.0
    r = D.knn_reference(row)
    i = int(np.flatnonzero(r['pinned'][:, 0] & r['pinned'][:, 1])[0])
    bad = idx.copy()
    bad[i, [0, 1]] = bad[i, [1, 0]]
    with pytest.raises(AssertionError):
        G._lists_fractions(row, dict(idx=bad, d2=d2))
    # mmd: the float64 sums pass; the sums of the instance one width short miss the gate
    row = _first('mix_rbf_sums', ns=6, shape=(130, 67, 36))
    X, Y = D.sets(row)
    sig, wts = D.mmd_widths(row)
    fr = G._mmd_fractions(row, dict(sums=np.array(D.mmd_reference(row))))
    assert max(fr.values()) == 0.0
    short = G._mmd_fractions(row, dict(sums=_mmd_ref.sums3(X, Y, sig[:5], wts[:5])))
    assert min(short.values()) > 1.0, short
