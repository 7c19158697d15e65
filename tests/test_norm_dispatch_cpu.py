"""The coverage table tests/_norm_dispatch.py against csrc/bn.hip and csrc/linear_bn.hip: every GGAN_LAUNCH site -- its label, the
kernel it launches and that kernel's template argument -- has a row, no row names a label the sources no longer launch, and no two
kernels share a label; every row's launches follow from a Python transcription of the dispatch predicates of ggan_bn_fwd_train,
ggan_bn_bwd_act, ggan_linear_bn_rows_fwd / _bwd and sp_plan; each threshold has a row on each side; the masked rows' inputs keep
their margin from the activation's kink.  Reads the project's own sources for names and constants only."""
import os
import re

import numpy as np

import _norm_dispatch as D
from _norm_dispatch import ROWS, row_id, dims

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graphical_gan_amd', 'csrc')
ENTRIES = ('bn_fwd', 'bn_bwd', 'sync', 'bwd_bwd', 'split', 'lin_fwd', 'lin_bwd')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _sources():
    return _read('bn.hip') + _read('linear_bn.hip')


# ---- labels against rows -----------------------------------------------------------------------------------------------------------------
_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*,\s*[^,]+,\s*[^,]+,\s*(\w+)(?:<([^()<>]*)>)?\s*,')


def source_sites(text):
    """-> {(label, kernel, template argument or None)} of every GGAN_LAUNCH site"""
    return {(m.group(1), m.group(2), m.group(3)) for m in _LAUNCH.finditer(text)}


def row_labels(rows=ROWS):
    return {l[0] for r in rows for l in r['launches']}


def uncovered(text):
    """-> (sites without a row, labels rows name that the text does not launch, labels that more than one kernel instance carries,
    sites whose label ends in _k or in <..> and is not the kernel's own name with its template argument)"""
    sites = source_sites(text)
    labels = row_labels()
    by_label = {}
    for label, kernel, targ in sites:
        by_label.setdefault(label, set()).add((kernel, targ))
    own = lambda kernel, targ: kernel + ('<%s>' % targ if targ is not None else '')
    return (sorted(s for s in sites if s[0] not in labels), sorted(labels - set(by_label)),
            sorted(l for l, ks in by_label.items() if len(ks) > 1),
            sorted(s for s in sites if (s[0].endswith('_k') or s[0].endswith('>') or s[2] is not None) and s[0] != own(s[1], s[2])))


def test_parser_reads_labels_kernels_and_template_arguments():
    text = ('    GGAN_LAUNCH("a_k", 0, 8.0 * N * C * HW, a_k, dim3(C), dim3(kThreads), 0, s, x, y);\n'
            '    if (K == 64) { GGAN_LAUNCH("b_k<4>", fl, bytes, b_k<4>, grid, block, shmem, s, P); }\n'
            '        case 2: GGAN_LAUNCH("c_k<2>", fl, bytes, c_k<2>, grid, block, shmem, s, P); break;\n'
            '    GGAN_LAUNCH("stats", 0, bytes, st_rows_k, dim3(cdiv(C, kSpCols), d.S, groups), dim3(kSpCols, kSpLanes), 0, s,\n        x, part, d);\n')
    assert source_sites(text) == {('a_k', 'a_k', None), ('b_k<4>', 'b_k', '4'), ('c_k<2>', 'c_k', '2'), ('stats', 'st_rows_k', None)}


def test_every_launch_has_a_row_and_every_row_a_launch():
    text = _sources()
    sites = source_sites(text)
    assert len(sites) == text.count('GGAN_LAUNCH('), 'a GGAN_LAUNCH site the parser does not read'
    missing, stale, shared, misnamed = uncovered(text)
    assert not missing, 'launched by bn.hip / linear_bn.hip without a row in tests/_norm_dispatch.py: %s' % missing
    assert not stale, 'rows of tests/_norm_dispatch.py name what the sources no longer launch: %s' % stale
    assert not shared, 'labels that more than one kernel instance carries: %s' % shared
    assert not misnamed, 'labels that claim a kernel name other than their own: %s' % misnamed
    labels = {s[0] for s in sites}
    assert {'linear_bn_rows_k<%d>' % r for r in range(1, 9)} | {'linear_bn_rows_bwd_k<%d>' % k for k in (4, 8, 16)} <= labels
    assert {D.REG, D.STREAM, D.ROWSF, D.R4S, D.R4L, D.BREG, D.BSTREAM, D.BROWS} <= labels
    assert all(len(l.encode()) < 48 for l in labels), 'a label longer than the 48-byte name field of ggan_prof_rec'


def test_a_scratch_copy_with_one_more_arm_is_caught():
    text = _sources()
    arm = 'GGAN_LAUNCH("bn_bwd_nchw_reg4_k<1024>", 0, 12.0 * N * C * HW, bn_bwd_nchw_reg4_k<1024>, dim3(C), dim3(1024), 0, s,'
    assert text.count(arm) == 1
    text = text.replace(arm, arm.replace('1024', '512') + ' x);\n    } else if (v4x) {\n        ' + arm)
    arm = 'case 8: GGAN_LAUNCH("linear_bn_rows_k<8>", fl, bytes, linear_bn_rows_k<8>, grid, block, shmem, s, P); break;'
    assert text.count(arm) == 1
    text = text.replace(arm, arm + '\n        ' + arm.replace('8', '9'))
    text += '    GGAN_LAUNCH("bn_fwd_nhwc_k", 0, bytes, bn_fwd_nhwc_k, dim3(C), dim3(kThreads), 0, s, x, y);\n'
    missing, stale, shared, misnamed = uncovered(text)
    assert missing == [('bn_bwd_nchw_reg4_k<512>', 'bn_bwd_nchw_reg4_k', '512'), ('bn_fwd_nhwc_k', 'bn_fwd_nhwc_k', None),
                       ('linear_bn_rows_k<9>', 'linear_bn_rows_k', '9')], missing
    assert (stale, shared, misnamed) == ([], [], []), (stale, shared, misnamed)


def test_a_scratch_copy_with_one_arm_fewer_is_caught():
    text = _sources()
    for site in ('GGAN_LAUNCH("bn_fwd_rows_k"', 'GGAN_LAUNCH("linear_bn_rows_bwd_k<16>"', 'GGAN_LAUNCH("bn_bwd_bwd"'):
        assert text.count(site) == 1
        text = text.replace(site, site.replace('GGAN_LAUNCH(', 'GGAN_LAUNCH_OFF('))
    missing, stale, shared, misnamed = uncovered(text)
    assert missing == [] and stale == ['bn_bwd_bwd', 'bn_fwd_rows_k', 'linear_bn_rows_bwd_k<16>'], (missing, stale)
    assert (shared, misnamed) == ([], []), (shared, misnamed)


def test_a_scratch_copy_with_a_shared_label_is_caught():
    """the labels as they were: four backward kernels under "bn_bwd_nchw", eight instances under "linear_bn_rows_k" """
    text = _sources()
    for name in (D.R4S, D.R4L, D.BREG, D.BSTREAM):
        assert text.count('GGAN_LAUNCH("%s"' % name) == 1
        text = text.replace('GGAN_LAUNCH("%s"' % name, 'GGAN_LAUNCH("bn_bwd_nchw"')
    missing, stale, shared, misnamed = uncovered(text)
    assert shared == ['bn_bwd_nchw'] and stale == sorted([D.R4S, D.R4L, D.BREG, D.BSTREAM]), (shared, stale)
    assert len(missing) == 4 and len(misnamed) == 2, (missing, misnamed)           # (the two reg4 sites carry a template argument)
    text = _sources().replace('GGAN_LAUNCH("linear_bn_rows_k<3>"', 'GGAN_LAUNCH("linear_bn_rows_k<2>"')
    missing, stale, shared, misnamed = uncovered(text)
    assert shared == ['linear_bn_rows_k<2>'] and stale == ['linear_bn_rows_k<3>'] and len(misnamed) == 1, (shared, stale, misnamed)


# ---- the dispatch, transcribed -------------------------------------------------------------------------------------------------------------
K = dict(kThreads=1024, kRegE=16, kCols=32, kSlices=16, kSyncThreads=256, kSpCols=64, kSpLanes=4, kSpThreads=256, kSpMerge=16, kSpTarget=1024,
         LB_COLS=32, LB_GROUPS=16)
V4_SMALL, V4_LARGE = 16 * 256, 16 * 1024


def cdiv(a, b):
    return -(-a // b)


def test_transcribed_constants_and_thresholds_are_the_sources():
    text = _sources()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(k\w+|LB_COLS|LB_GROUPS)\s*=\s*(\d+)\s*[,;]', text)}
    assert {k: found.get(k) for k in K} == K
    assert 'LB_THR = LB_COLS * LB_GROUPS' in text
    bn = _read('bn.hip')
    assert bn.count('HW > 1 && N * HW <= kRegE * kThreads') == 2                      # forward and backward
    assert bn.count('HW > 1 && v4 && N * HW <= 16 * 256)') == 1 and bn.count('HW > 1 && v4 && N * HW <= 16 * 1024)') == 1
    assert 'const bool v4 = (HW & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)gy) | ((uintptr_t)gx) | ((uintptr_t)mk.ref)) & 15) == 0;' in bn
    lin = _read('linear_bn.hip')
    assert 'switch (M / LB_GROUPS)' in lin and 'if (K == 64)' in lin and 'else if (K == 128)' in lin
    assert 'if (M > 128 || (M & 15) || (K & 3) || K > 256 || (N & 31)) return 1;' in lin
    assert 'if (M > 128 || (M & 15) || (K != 64 && K != 128 && K != 256) || (N & 31)) return 1;' in lin


def plan_fwd(N, C, HW):
    if HW > 1 and N * HW <= K['kRegE'] * K['kThreads']:
        return (D.REG, 1, (C,), (K['kThreads'],))
    if HW > 1:
        return (D.STREAM, 1, (C,), (K['kThreads'],))
    return (D.ROWSF, 1, (cdiv(C, K['kCols']),), (K['kCols'], K['kSlices']))


def plan_bwd(N, C, HW, aligned):
    """aligned: x, gy, gx and the mask's reference (where there is a mask) all sit on 16-byte boundaries"""
    v4 = HW % 4 == 0 and aligned
    if HW > 1 and v4 and N * HW <= V4_SMALL:
        return (D.R4S, 1, (C,), (256,))
    if HW > 1 and v4 and N * HW <= V4_LARGE:
        return (D.R4L, 1, (C,), (1024,))
    if HW > 1 and N * HW <= K['kRegE'] * K['kThreads']:
        return (D.BREG, 1, (C,), (K['kThreads'],))
    if HW > 1:
        return (D.BSTREAM, 1, (C,), (K['kThreads'],))
    return (D.BROWS, 1, (cdiv(C, K['kCols']),), (K['kCols'], K['kSlices']))


def sp_plan(N, C, HW, G):
    """-> (S, slab) of sp_plan"""
    Ng = N // G
    tiles = C if HW > 1 else cdiv(C, K['kSpCols'])
    want = max(1, K['kSpTarget'] // max(1, tiles * G))
    want = min(want, max(1, (Ng * HW) // 2048)) if HW > 1 else min(want, cdiv(Ng, K['kSpLanes']))
    want = max(1, min(want, Ng))
    slab = cdiv(Ng, want)
    return cdiv(Ng, slab), slab


def sp_apply_grid(elems):
    return min(cdiv(cdiv(elems, 4), 256), 2048)


def planned(row):
    """-> the launches the transcription derives for a row"""
    e = row['entry']
    if e in ('lin_fwd', 'lin_bwd'):
        M, Kk, N = row['shape']
        assert M <= 128 and M % 16 == 0 and N % 32 == 0
        grid, block = (N // K['LB_COLS'],), (K['LB_COLS'] * K['LB_GROUPS'],)
        if e == 'lin_fwd':
            assert Kk % 4 == 0 and Kk <= 256 and (M * (Kk + 4) + Kk * 32 + 16 * 32) * 4 <= 160 * 1024
            return (('linear_bn_rows_k<%d>' % (M // K['LB_GROUPS']), 1, grid, block),)
        assert (M * (Kk + 4) + M * 32 + 16 * 32) * 4 <= 160 * 1024
        return (('linear_bn_rows_bwd_k<%d>' % {64: 4, 128: 8, 256: 16}[Kk], 1, grid, block),)
    N, C, HW = dims(row)
    if e == 'bn_fwd':
        return (plan_fwd(N, C, HW),)
    if e == 'bn_bwd':
        off = row['off'] if row['act'] != 'none' else row['off'][:3]          # (no mask: the reference pointer is null)
        return (plan_bwd(N, C, HW, not any(off)),)
    if e == 'bwd_bwd':
        return (plan_fwd(N, C, HW), plan_bwd(N, C, HW, True), ('bn_bwd_bwd', 1, (C,), (K['kSyncThreads'],)))
    if e == 'sync':
        names = ('bn_sync_stats', 'bn_sync_apply') + (('bn_sync_bwd_stats', 'bn_sync_bwd_apply') if row['act'] in ('none',) + D.MASKS else ())
        return tuple((n, row['world'], (C,), (K['kSyncThreads'],)) for n in names)
    assert e == 'split'
    G = row['groups']
    S, _ = sp_plan(N, C, HW, G)
    lay = 'nchw' if HW > 1 else 'rows'
    sgrid = (C, S, G) if HW > 1 else (cdiv(C, K['kSpCols']), S, G)
    sblock = (K['kSpThreads'],) if HW > 1 else (K['kSpCols'], K['kSpLanes'])
    merge = (K['kSpCols'], K['kSpMerge'])
    apply_ = (sp_apply_grid(N * C * HW),)
    return (('bn_split_stats_' + lay, 1, sgrid, sblock), ('bn_split_merge', 1, (cdiv(C, K['kSpCols']), G), merge),
            ('bn_split_apply', 1, apply_, (256,)), ('bn_split_bwd_stats_' + lay, 1, sgrid, sblock),
            ('bn_split_bwd_merge', 1, (cdiv(C, K['kSpCols']),), merge), ('bn_split_bwd_apply', 1, apply_, (256,)))


def test_recorded_launches_follow_the_dispatch():
    for r in ROWS:
        assert planned(r) == r['launches'], (row_id(r), planned(r), r['launches'])


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for r in ROWS:
        assert r['entry'] in ENTRIES and r['act'] in D.ACTS, r
        assert r['alpha'] == (D.ALPHA if r['act'] == 'lrelu' else 0.0), r
        assert len(r['off']) == 4 and all(o in (0, 1) for o in r['off']) and (not any(r['off']) or r['entry'] == 'bn_bwd'), r
        assert not r['chansum'] or (r['entry'] == 'bn_bwd' and dims(r)[2] > 1), r
        assert r['entry'] in ('bn_fwd', 'sync', 'lin_fwd') or r['act'] in ('none',) + D.MASKS, r
        assert r['entry'] != 'split' or r['act'] in ('none',) + D.MASKS, r                        # (the split entry refuses tanh / sigmoid)
        for name, count, grid, block in r['launches']:
            assert count >= 1 and 1 <= len(grid) <= 3 and 1 <= len(block) <= 2 and int(np.prod(block)) <= 1024, r
        if r['entry'] in ('lin_fwd', 'lin_bwd'):
            assert 4 * max(r['shape'][0] * r['shape'][1], r['shape'][1] * r['shape'][2], r['shape'][0] * r['shape'][2]) <= 512 << 10, r
        else:
            N, C, HW = dims(r)
            assert 4 * N * C * HW <= 512 << 10 and (C % 2 == 1 or HW == 1), r                      # a few hundred KB; C small and odd
            assert r['world'] == 1 or (r['entry'] == 'sync' and N % r['world'] == 0), r
            assert r['const'] is None or 0 <= r['const'] < C, r


def test_table_keeps_the_cases_it_was_written_for():
    by = lambda e: [r for r in ROWS if r['entry'] == e]
    kern = lambda r: r['launches'][0][0]
    elems = lambda r: dims(r)[0] * dims(r)[2]
    hw = lambda r: dims(r)[2]
    fwd, bwd = by('bn_fwd'), by('bn_bwd')
    # every forward kernel with every epilogue, every backward kernel with every mask, chansum on each NCHW backward kernel
    for k in (D.REG, D.STREAM, D.ROWSF):
        assert {r['act'] for r in fwd if kern(r) == k} == set(D.ACTS), k
    for k in (D.R4S, D.R4L, D.BREG, D.BSTREAM, D.BROWS):
        assert {r['act'] for r in bwd if kern(r) == k} == {'none', 'lrelu', 'relu'}, k
        assert k == D.BROWS or any(r['chansum'] for r in bwd if kern(r) == k), k
    # each threshold from both sides: the last size on it or below it, the first size past it (one image more)
    al = [r for r in bwd if hw(r) > 1 and hw(r) % 4 == 0 and not any(r['off'])]
    for T, below, above in ((V4_SMALL, D.R4S, D.R4L), (V4_LARGE, D.R4L, D.BSTREAM)):
        assert any(elems(r) == T and kern(r) == below for r in al), T
        assert any(T < elems(r) <= T + hw(r) and kern(r) == above for r in al), T
    T = K['kRegE'] * K['kThreads']
    for rows, below, above in (([r for r in bwd if hw(r) % 4], D.BREG, D.BSTREAM), ([r for r in fwd if hw(r) > 1], D.REG, D.STREAM)):
        assert any(T - hw(r) < elems(r) <= T and kern(r) == below for r in rows), below
        assert any(T < elems(r) <= T + hw(r) and kern(r) == above for r in rows), above
    assert any(elems(r) == T and kern(r) == D.REG for r in fwd)
    # a non-power-of-two HW near the top of the FastDiv range, both directions
    assert all(any(hw(r) == 49 and T - 49 < elems(r) <= T for r in rows) for rows in (fwd, bwd))
    # alignment: one v4-eligible shape five times -- aligned, and each of x, gy, gx, y one float off on its own
    offs = [r for r in bwd if r['shape'] == (6, 5, 16)]
    assert sorted(r['off'] for r in offs) == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (1, 0, 0, 0)]
    assert all(r['act'] in D.MASKS and kern(r) == (D.BREG if any(r['off']) else D.R4S) for r in offs)
    # rows layout: one row per channel, a ragged tile with a ragged slice walk, a third shape -- both directions
    for rows in (fwd, bwd):
        assert {r['shape'] for r in rows if hw(r) == 1} == {(1, 5), (17, 33), (40, 64)}
        assert any(r['const'] is not None for r in rows)
    # sync: more than one trip of the 256-stride walk with a ragged tail, worlds 2 and 3, every epilogue
    sync = by('sync')
    per = lambda r: elems(r) // r['world']
    assert {per(r) for r in sync} == {315, 1030} and all(per(r) > 256 and per(r) % 256 for r in sync)
    assert {r['world'] for r in sync} == {2, 3} and {r['act'] for r in sync} == set(D.ACTS)
    assert {r['act'] for r in sync if len(r['launches']) == 4} == {'none', 'lrelu', 'relu'}
    assert {(elems(r), r['act']) for r in by('bwd_bwd')} == {(315, 'none'), (315, 'lrelu'), (1030, 'none'), (1030, 'lrelu')}
    # Linear + BatchNorm: every R at K = 20, N = 32; R = 5, 6, 7 again at K = 128, N = 96 with relu and without; every backward K
    lin = by('lin_fwd')
    assert {r['shape'] for r in lin if r['shape'][1:] == (20, 32)} == {(16 * R, 20, 32) for R in range(1, 9)}
    assert {(r['shape'], r['act']) for r in lin if r['shape'][1:] == (128, 96)} == {((16 * R, 128, 96), a) for R in (5, 6, 7) for a in ('relu', 'none')}
    assert {r['shape'][1] for r in by('lin_bwd')} == {64, 128, 256}
    assert {r['act'] for r in lin} == set(D.ACTS)
    assert {(dims(r)[2] > 1, r['act']) for r in by('split')} == {(l, a) for l in (True, False) for a in ('none', 'lrelu', 'relu')}


def test_masked_rows_keep_their_margin_from_the_kink():
    """the inputs test_norm_dispatch_gpu.py uploads (same seeds): no float64 pre-activation of a masked row within MARGIN of zero, the
    constant channel exactly constant, and every reference finite"""
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'split':                     # the float64 torch reference the GPU module compares with, without its activation
            import torch
            from test_ssgan_bn_gpu import _ref
            x, sc, of, gy = D.split_inputs(r, 7000 + idx)
            assert all(a.dtype == np.float32 and np.all(np.isfinite(a)) for a in (x, sc, of, gy)), row_id(r)
            v = _ref(*(torch.from_numpy(a).double() for a in (x, sc, of)), 'none', r['groups']).numpy()
            assert np.abs(v - D.split_preact(x, sc, of, r['groups'])).max() < 1e-12, row_id(r)
            if r['act'] in D.MASKS:
                assert np.abs(v).min() >= D.MARGIN, (row_id(r), np.abs(v).min())
            continue
        inp, ref = D.inputs(r, 7000 + idx)
        assert all(np.all(np.isfinite(v)) for v in ref.values()), row_id(r)
        assert all(v.dtype == np.float32 for v in inp.values()), row_id(r)
        if r['act'] in D.MASKS:
            assert D.margin(r, ref) >= D.MARGIN, (row_id(r), D.margin(r, ref))
        if r['const'] is not None:
            c = r['const']
            assert np.all(inp['x'][:, c] == 0.5) and np.all(ref['y'][:, c] == ref['y'][0, c].flat[0]), row_id(r)
            assert ref['save_mean'][c] == 0.5 and ref['save_invstd'][c] == 1.0 / np.sqrt(D.EPS)
