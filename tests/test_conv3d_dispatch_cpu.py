"""The coverage table tests/_conv3d_dispatch.py against csrc/conv3d.hip: every GGAN_LAUNCH site -- its label, the kernel it launches
and that kernel's template arguments -- has a row, no row names a label the source no longer launches, no two kernels share a label
and the data gradient has no AV4 = false instance; every row's launches and plan follow from a Python transcription of fill, ig_ok,
ig_split, the three entry points' plans and launch_splitk_reduce's choice; the rows cover the step counts, reduce kernels, workspace
caps and channel counts they were written for; and every FastDiv division a row's kernel forms is exact (brute force over the whole
numerator range), as it is for the boundary geometries ig_ok admits -- while the wide-volume geometry of FASTDIV_ROWS, which the rule
before this table admitted, is not.  Reads the project's own sources for names and constants only."""
import os
import re

import numpy as np

import _conv3d_dispatch as D
from _conv3d_dispatch import ROWS, FASTDIV_ROWS, row_id, geometry

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graphical_gan_amd', 'csrc')
IKS, IG_ROW_PAD, IG_COL_PAD = 32, 128, 64


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def cdiv(a, b):
    return -(-a // b)


# ---- labels against rows -----------------------------------------------------------------------------------------------------------------
_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*,\s*[^,]+,\s*[^,]+,\s*\(?(\w+)(?:<([^()<>]*)>)?\)?\s*,')


def source_sites(text):
    """-> {(label, kernel, template arguments or None)} of every GGAN_LAUNCH site"""
    return {(m.group(1), m.group(2), m.group(3)) for m in _LAUNCH.finditer(text)}


def row_labels(rows=None):
    return {l[0] for r in (ROWS + FASTDIV_ROWS if rows is None else rows) for l in r['launches']}


def uncovered(text):
    """-> (sites without a row, labels of this file's kernels that rows name and the text does not launch, labels that more than one
    kernel instance carries, sites whose label is not the kernel's own name with its template arguments, data-gradient instances with
    AV4 = false)"""
    sites = source_sites(text)
    labels = {l for l in row_labels() if l not in (D.RS, D.RK)}                # (the reduce kernels are launched from conv_corr.hip)
    by_label = {}
    for label, kernel, targ in sites:
        by_label.setdefault(label, set()).add((kernel, targ))
    own = lambda kernel, targ: kernel + ('<%s>' % targ if targ is not None else '')
    return (sorted(s for s in sites if s[0] not in labels), sorted(labels - set(by_label)), sorted(l for l, ks in by_label.items() if len(ks) > 1),
            sorted(s for s in sites if s[0] != own(s[1], s[2])),
            sorted(set(re.findall(r'conv3d_igemm_k<\s*2\s*,[^<>]*,\s*false\s*>', text))))


def test_parser_reads_labels_kernels_and_template_arguments():
    text = ('    if (av4) { GGAN_LAUNCH("a_k<1, 2, 2, true>", fl, 0, (a_k<1, 2, 2, true>), grid, dim3(256), 0, s, P); }\n'
            '    else if (i32) { GGAN_LAUNCH("b_k<uint32_t, 1>", 0, 8.0 * n, (b_k<uint32_t, 1>), dim3(blocks(n)), dim3(256), 0, s, g, x, col); }\n'
            '    GGAN_LAUNCH("c", 0, bytes, c_k, dim3(1), dim3(256), 0, s, x);\n')
    assert source_sites(text) == {('a_k<1, 2, 2, true>', 'a_k', '1, 2, 2, true'), ('b_k<uint32_t, 1>', 'b_k', 'uint32_t, 1'), ('c', 'c_k', None)}


def test_every_launch_has_a_row_and_every_row_a_launch():
    text = _read('conv3d.hip')
    sites = source_sites(text)
    assert len(sites) == text.count('GGAN_LAUNCH(') == 16, 'a GGAN_LAUNCH site the parser does not read'
    missing, stale, shared, misnamed, dgrad_false = uncovered(text)
    assert not missing, 'launched by conv3d.hip without a row in tests/_conv3d_dispatch.py: %s' % missing
    assert not stale, 'rows of tests/_conv3d_dispatch.py name what conv3d.hip no longer launches: %s' % stale
    assert not shared, 'labels that more than one kernel instance carries: %s' % shared
    assert not misnamed, 'labels that are not the kernel name with its template arguments: %s' % misnamed
    assert not dgrad_false, 'the data gradient always gathers 16-byte units: an AV4 = false instance is unreachable: %s' % dgrad_false
    labels = {s[0] for s in sites}
    want = {D.ig(0, 4, 1, True), D.ig(0, 4, 1, False), D.ig(0, 2, 2, True), D.ig(0, 2, 2, False), D.ig(1, 2, 2, True), D.ig(1, 2, 2, False),
            D.ig(2, 4, 1, True), D.ig(2, 2, 2, True)}
    assert labels == want | {'%s_k<%s, %d>' % (k, it, v) for k in ('im2col3d', 'col2im3d') for it in ('uint32_t', 'size_t') for v in (4, 1)}
    assert all(l.startswith(('conv3d_igemm_k<', 'im2col3d', 'col2im3d')) for l in labels)         # (the old labels stay prefixes)
    assert all(len(l.encode()) < 48 for l in labels), 'a label longer than the 48-byte name field of ggan_prof_rec'
    # the launches of the reduction's second stage are conv_corr.hip's
    assert {D.RS, D.RK} <= {s[0] for s in source_sites(_read('conv_corr.hip'))}
    # not-run is accepted for the four 64-bit index instances (two kernels) and for nothing else
    not_run = [r for r in ROWS if r['run']]
    assert sorted(r['launches'][0][0] for r in not_run) == sorted(D.SIZE_T_LABELS) and all(r['run'] == D.NOT_RUN for r in not_run)
    ran = row_labels([r for r in ROWS + FASTDIV_ROWS if not r['run']])
    assert ran == (labels - set(D.SIZE_T_LABELS)) | {D.RS, D.RK}, sorted(labels - ran)


def test_a_scratch_copy_with_one_more_or_one_fewer_arm_or_a_shared_label_is_caught():
    text = _read('conv3d.hip')
    arm = 'GGAN_LAUNCH("conv3d_igemm_k<2, 4, 1, true>", fl, 0, (conv3d_igemm_k<2, 4, 1, true>), grid, dim3(256), 0, s, P);'
    assert text.count(arm) == 1
    more = text.replace(arm, arm + ' }\n    else if (x) { ' + arm.replace('true', 'false'))
    missing, stale, shared, misnamed, dgrad_false = uncovered(more)
    assert missing == [('conv3d_igemm_k<2, 4, 1, false>', 'conv3d_igemm_k', '2, 4, 1, false')] and dgrad_false == ['conv3d_igemm_k<2, 4, 1, false>']
    assert (stale, shared, misnamed) == ([], [], [])
    missing, stale, shared, misnamed, dgrad_false = uncovered(text.replace(arm, ''))
    assert (missing, stale, shared, misnamed, dgrad_false) == ([], ['conv3d_igemm_k<2, 4, 1, true>'], [], [], [])
    old = text
    for it in ('uint32_t', 'size_t'):
        for v in (4, 1):
            assert old.count('GGAN_LAUNCH("im2col3d_k<%s, %d>"' % (it, v)) == 1
            old = old.replace('GGAN_LAUNCH("im2col3d_k<%s, %d>"' % (it, v), 'GGAN_LAUNCH("im2col3d"')
    missing, stale, shared, misnamed, dgrad_false = uncovered(old)
    assert shared == ['im2col3d'] and len(missing) == 4 and len(stale) == 4 and len(misnamed) == 4, (missing, stale, shared, misnamed)


# ---- the dispatch, transcribed -------------------------------------------------------------------------------------------------------------
def test_transcribed_constants_and_predicates_are_the_sources():
    text = _read('conv3d.hip')
    for line in ('constexpr int IKS = 32;', 'constexpr size_t IG_ROW_PAD = 128, IG_COL_PAD = 64;',
                 'if (rows >= (1u << 24) || vox >= (1u << 24) || K >= (1u << 16) || (g.Co & 3)) return false;',
                 'if (xb >= 0x7FFFFFF0ull || yb >= 0x7FFFFFF0ull || K * g.Co * 4 >= 0x7FFFFFF0ull) return false;',
                 'if ((g.Ci & 3) || g.sl > 2 || g.s > 2 || g.Ci < 16) return false;',
                 'if ((count + pad) * (size_t)d[i] >= (1ull << 32)) return false;',
                 'return fd_chain_ok(rows, IG_ROW_PAD, g.Wo, g.Ho, g.Lo) && fd_chain_ok(K, IG_COL_PAD, g.Ci, g.k, g.k);',
                 'return fd_chain_ok(rows, IG_ROW_PAD, g.Wo, g.Ho, g.Lo) && fd_chain_ok((size_t)tl * t * t * g.Co, IG_COL_PAD, g.Co, t, t);',
                 'if (tiles < target / 2) {', 'const int max_sk = kred / (4 * IKS);', 'if (sk > 512) sk = 512;',
                 'while (sk > 1 && (size_t)sk * out_elems > ws_floats) --sk;',
                 'P.SK = ig_split(gx * gy, Q.K, out_elems, scratch ? wsb / 4 : 0, 512);',
                 'P.SK = ig_split(gx * gyt, Q.M, out_elems, scratch ? wsb / 4 : 0, 1024);',
                 'const bool wide = g.Co > 32;', 'const bool wide = g.Ci > 32;', 'const int BM = wide ? 64 : 128, BN = wide ? 64 : 32;',
                 'const int gx = cdiv(g.Co, 64), gyt = cdiv(Q.K, 64);', 'if (Q.M == 0) continue;',
                 'return ig_launch_dgrad(P, dim3(cdiv(max_m, BM), cdiv(g.Ci, BN), nc), wide, s, fl);'):
        assert line in text, line
    assert text.count('i32 = n < 0xF0000000ull;') == 2 and 'return (int)(b > 32768 ? 32768 : (b < 1 ? 1 : b));' in text
    corr = _read('conv_corr.hip')
    assert 'if (SK >= 8 && elems + tail <= 65536) {' in corr and 'dim3((int)((elems + tail + 63) / 64)), dim3(256)' in corr
    assert 'size_t b = (elems + tail + 255) / 256;\n    if (b > 2048) b = 2048;' in corr
    with open(os.path.join(CSRC, '..', '..', 'include', 'ggan.h')) as f:
        assert '#define GGAN_WS_RESERVED %d\n' % D.WS_RESERVED in f.read()
    assert 'f.mul = (d <= 1) ? 0u : (uint32_t)((0x100000000ull / d) + 1ull);' in _read('conv.h')
    assert 'fdiv(uint32_t n, FastDiv f) { return f.d <= 1 ? n : __umulhi(n, f.mul); }' in _read('conv.h')


def fd_chain_ok(count, pad, ds):
    for d in ds:
        if d <= 1:
            continue
        if (count + pad) * d >= 1 << 32:
            return False
        count = cdiv(count, d)
    return True


def source_enforces_fastdiv():
    """ig_ok of conv3d.hip as it stands ends both of its branches in the two fd_chain_ok chains"""
    text = _read('conv3d.hip')
    body = text[text.index('bool ig_ok(const C3& g, int kind) {'):]
    body = body[:body.index('\n}\n')]
    return body.count('return fd_chain_ok(rows, IG_ROW_PAD, g.Wo, g.Ho, g.Lo) && fd_chain_ok(') == 2


def ig_ok(dims, kind, fastdiv_rule=None):
    """ig_ok of conv3d.hip; fastdiv_rule=False: the rule before FastDiv's contract was enforced (the default: what the source does)"""
    if fastdiv_rule is None:
        fastdiv_rule = source_enforces_fastdiv()
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    (Lo, Ho, Wo), _ = geometry(dims)
    rows, vox, K = N * Lo * Ho * Wo, N * L * H * W, fl * fs * fs * Ci
    if vox * Ci * 4 >= 0x7FFFFFF0 or rows * Co * 4 >= 0x7FFFFFF0 or K * Co * 4 >= 0x7FFFFFF0:
        return False
    if rows >= 1 << 24 or vox >= 1 << 24 or K >= 1 << 16 or Co % 4:
        return False
    if kind == 2:
        if Ci % 4 or sl > 2 or s > 2 or Ci < 16:
            return False
        tl, t = cdiv(fl, sl), cdiv(fs, s)
        return not fastdiv_rule or (fd_chain_ok(rows, IG_ROW_PAD, (Wo, Ho, Lo)) and fd_chain_ok(tl * t * t * Co, IG_COL_PAD, (Co, t, t)))
    return not fastdiv_rule or (fd_chain_ok(rows, IG_ROW_PAD, (Wo, Ho, Lo)) and fd_chain_ok(K, IG_COL_PAD, (Ci, fs, fs)))


def ig_split(tiles, kred, out_elems, ws_floats, target):
    sk = 1
    if tiles < target // 2:
        sk = min(target // max(tiles, 1), kred // (4 * IKS), 512)
        while sk > 1 and sk * out_elems > ws_floats:
            sk -= 1
    return max(sk, 1)


def reduce_launch(SK, elems):
    if SK >= 8 and elems <= 65536:
        return (D.RS, 1, (cdiv(elems, 64), 1, 1), 256)
    return (D.RK, 1, (min(cdiv(elems, 256), 2048), 1, 1), 256)


def dgrad_classes(dims):
    """the residue classes of ggan_conv3d_dgrad that have rows -> [dict(M, K, R=(RL, RH, RW), T=(TL, TH, TW))]"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    _, (pl, ph, pw) = geometry(dims)

    def axis(c, n, k, st, pad):
        d0 = (c + pad) % st
        return (cdiv(k - d0, st) if d0 < k else 0, cdiv(n - c, st) if c < n else 0)          # (taps, rows)
    out = []
    for cl in range(sl):
        for ch in range(s):
            for cw in range(s):
                (tl, rl), (th, rh), (tw, rw) = axis(cl, L, fl, sl, pl), axis(ch, H, fs, s, ph), axis(cw, W, fs, s, pw)
                if N * rl * rh * rw:
                    out.append(dict(M=N * rl * rh * rw, K=tl * th * tw * Co, R=(rl, rh, rw), T=(tl, th, tw)))
    return out


def blocks(n):
    return min(max(cdiv(n, 256), 1), 32768)


def planned(row):
    """-> (launches, plan) the transcription derives for a row"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = row['dims']
    (Lo, Ho, Wo), _ = geometry(row['dims'])
    M, K, e = N * Lo * Ho * Wo, fl * fs * fs * Ci, row['entry']
    if e in ('im2col', 'col2im'):
        n = M * K if e == 'im2col' else N * L * H * W * Ci
        v = 4 if Ci % 4 == 0 and not row['off'] else 1
        it = 'uint32_t' if n < 0xF0000000 else 'size_t'
        return (('%s3d_k<%s, %d>' % (e, it, v), 1, (blocks(n // v), 1, 1), 256),), None
    if row['refused'] or not ig_ok(row['dims'], D.KIND[e]):
        return (), None
    ws = row['ws'] or 0
    if e == 'fwd':
        wide = Co > 32
        BM, BN = (64, 64) if wide else (128, 32)
        gx, gy = cdiv(Co, BN), cdiv(M, BM)
        kred, elems = K, M * Co
        SK = ig_split(gx * gy, kred, elems, ws, 512)
        label, grid = D.ig(0, 2 if wide else 4, 2 if wide else 1, Ci % 4 == 0), (gy, gx)
    elif e == 'wgrad':
        gx, gyt = cdiv(Co, 64), cdiv(K, 64)
        kred, elems = M, K * Co
        SK = ig_split(gx * gyt, kred, elems, ws, 1024)
        label, grid = D.ig(1, 2, 2, Ci % 4 == 0), (gyt, gx)
    else:
        cls = dgrad_classes(row['dims'])
        wide = Ci > 32
        BM, BN = (64, 64) if wide else (128, 32)
        grid = (cdiv(max(c['M'] for c in cls), BM), cdiv(Ci, BN), len(cls))
        return ((D.ig(2, 2 if wide else 4, 2 if wide else 1, True), 1, grid, 256),), dict(nc=len(cls), classes=tuple((c['M'], c['K']) for c in cls))
    kps = cdiv(cdiv(kred, SK), IKS) * IKS
    SK = cdiv(kred, kps)
    launches = ((label, 1, grid + (SK,), 256),) + ((reduce_launch(SK, elems),) if SK > 1 else ())
    return launches, dict(SK=SK, kps=kps, steps=cdiv(min(kps, kred), IKS), last=kred - (SK - 1) * kps)


def test_recorded_launches_and_plans_follow_the_dispatch():
    for r in ROWS:
        assert planned(r) == (r['launches'], r['plan']), (row_id(r), planned(r), r['launches'], r['plan'])
    for r in FASTDIV_ROWS:                 # the patch route of functional.conv3d: the layout kernels' launches, no implicit kernel
        assert not any(ig_ok(r['dims'], k) for k in range(3)), row_id(r)
        lay = tuple(planned(dict(r, entry=e))[0][0] for e in (('im2col', 'col2im') if r['entry'] == 'dgrad' else ('im2col',)))
        assert lay == r['launches'], (row_id(r), lay)


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS + FASTDIV_ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    operands = dict(fwd=('x', 'w', 'y'), wgrad=('x', 'gy', 'gw'), dgrad=('gy', 'w', 'gx'), im2col=('x', 'col'), col2im=('col', 'gx'))
    for r in ROWS + FASTDIV_ROWS:
        N, L, H, W, Ci, Co, fl, fs, sl, s = r['dims']
        assert r['entry'] in D.ENTRY and r['act'] in D.ACTS and len(r['dims']) == 10 and min(r['dims']) >= 1, r
        assert r['alpha'] == (D.ALPHA if r['act'] == 'lrelu' else 0.0), r
        assert r['entry'] == 'fwd' or (not r['bias'] and r['act'] == 'none'), r
        assert r['entry'] in ('fwd', 'wgrad') or r['ws'] is None, r
        assert set(r['off']) <= set(operands[r['entry']]), r
        assert r['refused'] == (r['launches'] == ()) and (r['plan'] is None) == (r['refused'] or r['entry'] in ('im2col', 'col2im') or r['exact']), r
        assert all(len(l[2]) == 3 and l[3] == 256 and l[1] >= 1 for l in r['launches']), r
        assert r['exact'] == (r in FASTDIV_ROWS), r
        if not r['exact'] and not r['run']:                                         # every tensor of an ordinary row stays below 1 MB
            (Lo, Ho, Wo), _ = geometry(r['dims'])
            assert 4 * max(N * L * H * W * Ci, N * Lo * Ho * Wo * max(Co, fl * fs * fs * Ci if r['entry'] in ('im2col', 'col2im') else 0),
                           fl * fs * fs * Ci * Co) <= 1 << 20, row_id(r)


def _units_straddle_tw_and_th(Ci, fl, fs):
    """AV4 = false: some unit of four consecutive k crosses a tw wrap and a th wrap"""
    col = lambda k: ((k // Ci) // fs // fs, (k // Ci) // fs % fs, (k // Ci) % fs)
    for k in range(0, fl * fs * fs * Ci - 3, 4):
        taps = [col(k + j) for j in range(4)]
        if any(a[1] == b[1] and a[2] != b[2] for a, b in zip(taps, taps[1:])) and any(a[0] != b[0] for a, b in zip(taps, taps[1:])):
            return True
    return False


def test_table_keeps_the_cases_it_was_written_for():
    ok = [r for r in ROWS if not r['refused'] and not r['run']]
    by = lambda e: [r for r in ok if r['entry'] == e]
    kern = lambda r: r['launches'][0][0]
    fwd, wg, dg = by('fwd'), by('wgrad'), by('dgrad')
    ci, co = (lambda r: r['dims'][4]), (lambda r: r['dims'][5])
    # steps per split 1..5 at SK = 1 for each kind (the data gradient: of its only class)
    for rows in (fwd, wg):
        assert {1, 2, 3, 4, 5} <= {r['plan']['steps'] for r in rows if r['plan']['SK'] == 1 and ci(r) == 4}
    assert {1, 2, 3, 4, 5} <= {cdiv(r['plan']['classes'][0][1], IKS) for r in dg if r['plan']['nc'] == 1 and ci(r) == 16}
    assert {r['dims'][6:8] for r in fwd if ci(r) == 4 and co(r) == 12 and r['plan']['SK'] == 1} >= {(5, 1), (1, 3), (2, 3), (2, 4), (4, 3)}
    # both reduce kernels behind each split kind; an epilogue that moves to the reduce and its direct twin; a short last split
    for rows in (fwd, wg):
        assert {r['launches'][1][0] for r in rows if r['plan']['SK'] > 1} == {D.RS, D.RK}
        assert any(r['plan']['SK'] > 1 and r['plan']['last'] < r['plan']['kps'] for r in rows)
        # one geometry with a generous workspace, a cap that leaves SK > 1, a cap that leaves 1, and no workspace
        caps = {}
        for r in rows:
            caps.setdefault((r['dims'], r['bias'], r['act']), set()).add((r['ws'], r['plan']['SK']))
        assert any(len(v) == 4 and {w for w, _ in v} >= {D.BIG, None} and len({k for _, k in v}) == 3 and
                   sorted(k for w, k in v if w not in (D.BIG, None))[0] == 1 for v in caps.values()), caps
    assert any(r['plan']['SK'] > 1 and r['launches'][1][0] == D.RK and r['plan']['SK'] >= 8 for r in fwd)          # (by elems > 65536)
    assert any(r['plan']['SK'] > 1 and r['launches'][1][0] == D.RK and r['plan']['SK'] < 8 for r in fwd)
    for split in (True, False):
        assert any(r['bias'] and r['act'] == 'lrelu' and (r['plan']['SK'] > 1) == split for r in fwd), split
    # AV4 = false at every thin channel count, K % 4 != 0, a unit across a tw wrap and a th wrap
    for rows in (fwd, wg):
        assert {ci(r) for r in rows if 'false' in kern(r)} == {1, 2, 3, 5, 6} and all(co(r) % 4 == 0 for r in rows)
        assert any(r['dims'][4:8] == (3, co(r), 3, 3) for r in rows)                  # K = 81
        assert any('false' in kern(r) and _units_straddle_tw_and_th(ci(r), *r['dims'][6:8]) for r in rows)
    assert {kern(r) for r in fwd} == {D.ig(0, wm, wn, a) for wm, wn in ((4, 1), (2, 2)) for a in (True, False)}
    assert {kern(r) for r in wg} == {D.ig(1, 2, 2, True), D.ig(1, 2, 2, False)} and {kern(r) for r in dg} == {D.ig(2, 4, 1, True), D.ig(2, 2, 2, True)}
    # data gradient: classes without rows (nc 4 and 2), unequal taps, classes without a tap, ragged channel counts, K below one step
    assert any(r['dims'][1] == 1 and r['dims'][8] == 2 and r['plan']['nc'] == 4 for r in dg)
    assert any(r['dims'][3] == 1 and r['dims'][9] == 2 and r['plan']['nc'] == 2 for r in dg)
    assert any(r['dims'][6] == 3 and r['dims'][8] == 2 and len({k for _, k in r['plan']['classes']}) > 1 for r in dg)
    assert any(r['dims'][6:8] == (1, 1) and sum(k == 0 for _, k in r['plan']['classes']) == 7 for r in dg)
    assert {16, 20, 36} <= {ci(r) for r in dg} and any(co(r) == 4 and max(k for _, k in r['plan']['classes']) < IKS for r in dg)
    # SAME padding (0, 1) and (1, 2) along each axis, a filter longer than the volume -- for every kind
    for rows in (fwd, wg, dg):
        pads = set()
        for r in rows:
            N, L, H, W, Ci, Co, fl, fs, sl, s = r['dims']
            (Lo, Ho, Wo), p = geometry(r['dims'])
            tot = ((Lo - 1) * sl + fl - L, (Ho - 1) * s + fs - H, (Wo - 1) * s + fs - W)
            pads |= {(ax, p[ax], tot[ax] - p[ax], (sl, s, s)[ax]) for ax in range(3)}
            pads |= {'longer'} if fl > L else set()
        assert {(0, 1, 2, 1), (1, 1, 2, 1), (2, 1, 2, 1), (1, 0, 1, 1), (2, 0, 1, 1), (1, 0, 1, 2), (2, 0, 1, 2), (0, 0, 1, 2), 'longer'} <= pads, pads
    # ragged tiles: some row of each instance has a row count and a column count that are no multiple of its tile
    def ragged(r):
        N, L, H, W, Ci, Co, fl, fs, sl, s = r['dims']
        (Lo, Ho, Wo), _ = geometry(r['dims'])
        tm, tn = (64, 64) if ', 2, 2, ' in kern(r) else (128, 32)
        m, n = dict(fwd=(N * Lo * Ho * Wo, Co), wgrad=(fl * fs * fs * Ci, Co), dgrad=(dgrad_classes(r['dims'])[0]['M'], Ci))[r['entry']]
        return bool(m % tm and n % tn)
    for k in {kern(r) for r in fwd + wg + dg}:
        assert any(ragged(r) for r in fwd + wg + dg if kern(r) == k), k
    # the layout kernels: V = 4, V = 1 by the channel count, V = 1 by either operand's base
    for e in ('im2col', 'col2im'):
        got = {(kern(r), r['dims'][4] % 4 == 0, r['off']) for r in by(e)}
        other = 'x' if e == 'im2col' else 'gx'
        assert got == {('%s3d_k<uint32_t, 4>' % e, True, ()), ('%s3d_k<uint32_t, 1>' % e, False, ()), ('%s3d_k<uint32_t, 1>' % e, True, (other,)),
                       ('%s3d_k<uint32_t, 1>' % e, True, ('col',))}, got
    # argument checks: each operand of each entry off its boundary, and a geometry ggan_conv3d_igemm_ok rejects
    ref = [r for r in ROWS if r['refused']]
    for e, ops in (('fwd', ('x', 'w', 'y')), ('wgrad', ('x', 'gy', 'gw')), ('dgrad', ('gy', 'w', 'gx'))):
        mine = [r for r in ref if r['entry'] == e]
        assert {r['off'] for r in mine if ig_ok(r['dims'], D.KIND[e])} == {(o,) for o in ops}, e
        assert any(not r['off'] and not ig_ok(r['dims'], D.KIND[e]) for r in mine), e
    assert [(r['entry'], r['dims'][4]) for r in FASTDIV_ROWS] == [('fwd', 4), ('wgrad', 4), ('dgrad', 16)]
    assert all(r['dims'][:4] == (1, 1, 258, 4096) and r['dims'][5:] == (4, 1, 1, 1, 1) for r in FASTDIV_ROWS)


# ---- FastDiv -----------------------------------------------------------------------------------------------------------------------------------
def fdiv(n, d):
    """make_fastdiv + fdiv of conv.h on a uint32 array"""
    if d <= 1:
        return n.astype(np.uint64)
    mul = ((1 << 32) // d + 1) & 0xFFFFFFFF
    return (n.astype(np.uint64) * np.uint64(mul)) >> np.uint64(32)


def first_wrong(bound, d):
    """the first n < bound with fdiv(n, d) != n // d, or None"""
    n = np.arange(bound, dtype=np.uint64)
    bad = np.flatnonzero(fdiv(n, d) != n // np.uint64(max(d, 1)))
    return int(bad[0]) if bad.size else None


def chains(dims, kind):
    """every (numerator bound, divisor) pair the kernels of `kind` form for the geometry: the bound is exclusive and includes the rows
    and columns the last tile and the last k-step reach past M and K"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    (Lo, Ho, Wo), _ = geometry(dims)
    M, K = N * Lo * Ho * Wo, fl * fs * fs * Ci
    out = []

    def chain(bound, ds):
        for d in ds:
            out.append((bound, d))
            bound = cdiv(bound, max(d, 1))
    if kind == 0:
        BM = 64 if Co > 32 else 128
        chain(cdiv(M, BM) * BM, (Wo, Ho, Lo))                        # ig_row(m0 + ..) of the tile's rows
        chain(cdiv(K, IKS) * IKS, (Ci, fs, fs))                      # ig_col(k0 + ..) of a step's columns
    elif kind == 1:
        chain(cdiv(M, IKS) * IKS, (Wo, Ho, Lo))                      # ig_row of a step's rows (up to ke + 31)
        chain(cdiv(K, 64) * 64, (Ci, fs, fs))                        # ig_col of the tile's columns
    else:
        BM = 64 if Ci > 32 else 128
        for c in dgrad_classes(dims):
            chain(cdiv(c['M'], BM) * BM, c['R'][::-1])
            chain(cdiv(c['K'], IKS) * IKS, (Co,) + tuple(max(t, 1) for t in c['T'][:0:-1]))
    return out


def test_chains_stay_inside_the_pads_of_ig_ok():
    """the numerators transcribed above never pass what ig_ok bounds: rows below M + IG_ROW_PAD, columns below K + IG_COL_PAD, and the
    divisors of a data-gradient class never pass those of the volume"""
    for r in ROWS:
        if r['entry'] not in D.KIND or r['refused']:
            continue
        N, L, H, W, Ci, Co, fl, fs, sl, s = r['dims']
        (Lo, Ho, Wo), _ = geometry(r['dims'])
        k = D.KIND[r['entry']]
        top = (((N * Lo * Ho * Wo, IG_ROW_PAD, (Wo, Ho, Lo)), (fl * fs * fs * Ci, IG_COL_PAD, (Ci, fs, fs))) if k < 2 else
               ((N * Lo * Ho * Wo, IG_ROW_PAD, (Wo, Ho, Lo)), (cdiv(fl, sl) * cdiv(fs, s) ** 2 * Co, IG_COL_PAD, (Co, cdiv(fs, s), cdiv(fs, s)))))
        pairs = chains(r['dims'], k)
        assert len(pairs) % 6 == 0, row_id(r)
        for i, (bound, d) in enumerate(pairs):
            count, pad, ds = top[(i // 3) % 2]
            for dd in ds[:i % 3]:
                count = cdiv(count, max(dd, 1))
            assert bound <= count + pad and d <= ds[i % 3], (row_id(r), i, bound, d, count, pad, ds)


BOUNDARY = [  # (dims, kinds admitted): on each side of the condition ig_ok enforces, by rows and by columns
    ((1, 1, 255, 4096, 4, 4, 1, 1, 1, 1), (0, 1)), ((1, 1, 256, 4096, 4, 4, 1, 1, 1, 1), ()),
    ((1, 1, 255, 4096, 16, 4, 1, 1, 1, 1), (0, 1, 2)), ((1, 1, 256, 4096, 16, 4, 1, 1, 1, 1), ()),
    ((1, 1, 3, 32768, 1, 4, 1, 1, 1, 1), (0, 1)), ((1, 1, 4, 32768, 1, 4, 1, 1, 1, 1), ()),
    ((1, 1, 510, 8192, 16, 4, 1, 1, 1, 2), (0, 1, 2)), ((1, 1, 512, 8192, 16, 4, 1, 1, 1, 2), ()),
    ((1, 2, 2, 2, 65504, 4, 1, 1, 1, 1), (0, 1, 2)), ((1, 2, 2, 2, 65508, 4, 1, 1, 1, 1), (2,)),
    ((1, 2, 2, 2, 16, 65504, 1, 1, 1, 1), (0, 1, 2)), ((1, 2, 2, 2, 16, 65508, 1, 1, 1, 1), (0, 1)),
]


def test_every_admitted_division_is_exact():
    """brute force over the whole numerator range of every (range, divisor) pair: the rows' geometries and the boundary geometries"""
    seen = {}
    geoms = [(r['dims'], D.KIND[r['entry']]) for r in ROWS if r['entry'] in D.KIND and not r['refused']]
    assert all(ig_ok(dims, k) for dims, k in geoms)
    geoms += [(dims, k) for dims in [r['dims'] for r in FASTDIV_ROWS] + [b[0] for b in BOUNDARY] for k in range(3) if ig_ok(dims, k)]
    for dims, k in geoms:
        for bound, d in chains(dims, k):
            if (bound, d) not in seen:
                seen[(bound, d)] = first_wrong(bound, d)
            assert seen[(bound, d)] is None, 'ig_ok admits %s for kind %d: n / %d is wrong at n = %d < %d' % (dims, k, d, seen[(bound, d)], bound)
            assert bound * d < 1 << 32, (dims, k, bound, d)               # (FastDiv's documented contract, which is sufficient, not necessary)
    for dims, kinds in BOUNDARY:
        assert tuple(k for k in range(3) if ig_ok(dims, k)) == kinds, (dims, [ig_ok(dims, k) for k in range(3)])


def test_the_wide_volume_was_admitted_and_is_inexact():
    """FASTDIV_ROWS: the rule without fd_chain_ok admits the geometry, and its first division, row / 4096, is wrong from 1 052 671 on --
    256 * 4096 + 4095, the last voxel of the 257th row: the quotient comes out one too large, ig_row decodes rw = -1"""
    for r in FASTDIV_ROWS:
        k = D.KIND[r['entry']]
        assert ig_ok(r['dims'], k, fastdiv_rule=False) and not ig_ok(r['dims'], k)
        bound, d = chains(r['dims'], k)[0]
        assert d == 4096 and bound >= 258 * 4096
        assert first_wrong(bound, d) == 1052671 == 256 * 4096 + 4095
        n = np.arange(258 * 4096, dtype=np.uint64)
        wrong = np.flatnonzero(fdiv(n, d) != n // np.uint64(d))
        assert wrong.tolist() == [1052671, 1056767] and fdiv(n[wrong], d).tolist() == [257, 258]        # the last voxel of rows 256 and 257
    for d, n in ((4096, 1052671), (1024, 4195327), (512, 8389119), (1000, 6100999)):
        assert first_wrong(n + 1, d) == n, (d, first_wrong(n + 1, d))
