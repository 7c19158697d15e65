"""The coverage table tests/_cost_dispatch.py against csrc/losses.hip and cost_head.h, without a GPU: every GGAN_LAUNCH label and every
kernel of losses.hip has a row and the rows name nothing else; the constants planned() copies are the source's; every row's launches
follow from planned(); the rows reach a second trip of every strided loop, every limit, every optional pointer both ways and both
heads; the float32 restatement of the kernels (run32) passes every bound on every row, while each wrong kernel of MUTANTS misses a
bound or breaks a bitwise stage on the row named here; and the calls of REJECTED answer before any launch."""
import os
import re

import numpy as np
import pytest

import _cost_dispatch as D
from _cost_dispatch import ROWS, row_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7000


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _source():
    return _read('graphical_gan_amd', 'csrc', 'losses.hip')


_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*(?:"([^"]+)"|(\w+))\s*,.*?,\s*(\w+_k)\s*,\s*dim3\(([^;]*?)\),\s*dim3\((\w+)\)', re.S)
# the launch sites that take their label from a parameter, and the labels their callers hand over
_LABEL_ARGS = {'rows_label': ('mmd2_rows', 'mmd2u_rows'), 'label': ('mmd2_bwd', 'mmd2u_bwd')}


def sites(text):
    """-> {(label, kernel)} of every GGAN_LAUNCH site of the text"""
    out = set()
    found = list(_LAUNCH.finditer(text))
    assert len(found) == text.count('GGAN_LAUNCH('), (len(found), text.count('GGAN_LAUNCH('))
    for s in found:
        for label in ((s.group(1),) if s.group(1) else _LABEL_ARGS[s.group(2)]):
            assert not s.group(1) is None or '"%s"' % label in text, label
            out.add((label, s.group(3)))
    return out


def row_sites(rows):
    return {(l[0], k) for r in rows for l in r['launches'] for k in l[4].split('+')}


_INPUTS = {}


def _inp(i):
    if i not in _INPUTS:
        _INPUTS[i] = D.inputs(ROWS[i], SEED + i)
    return _INPUTS[i]


def _index(rid):
    return [row_id(r) for r in ROWS].index(rid)


# ---- launch sites, kernels, constants, the plan ---------------------------------------------------------------------------------------------
def test_every_site_and_kernel_has_a_row_and_every_row_a_site():
    text = _source()
    assert sites(text) == row_sites(ROWS), (sorted(sites(text) - row_sites(ROWS)), sorted(row_sites(ROWS) - sites(text)))
    kernels = D.source_kernels(text)
    assert len(kernels) == 21 and kernels == sorted({k for _, k in row_sites(ROWS)}), kernels
    assert len(re.findall(r'^int ggan_\w+\(', text, flags=re.M)) == 21          # (the exported entry points of this unit)
    # what the profiler can show of a row is what planned() derives: every kernel appears in some row's plan
    assert {k for r in ROWS for l in D.planned(r) for k in l[4].split('+')} == set(kernels)
    # every check of every row is attributed to a kernel of the source
    assert {k for r in ROWS for k in D.kernels_of(r).values()} <= set(kernels)


def test_a_scratch_copy_with_a_new_or_a_lost_site_is_caught():
    text = _source()
    site = 'GGAN_LAUNCH("gp_penalty"'
    assert text.count(site) == 1
    assert ('gp_penalty2', 'gp_pen_k') in sites(text.replace(site, 'GGAN_LAUNCH("gp_penalty2"')) - row_sites(ROWS)
    assert ('gp_penalty', 'gp_pen_k') in sites(text) - row_sites([r for r in ROWS if r['entry'] != 'gp'])


def test_transcribed_constants_are_the_sources():
    text, hdr = _source(), _read('include', 'ggan.h')
    assert '#define GGAN_BCE_MAX %d' % D.BCE_MAX in hdr and '#define GGAN_BCE_HEADS %d' % D.BCE_HEADS in hdr
    assert '#define GGAN_HEAD_BCE_MAX_ROWS %d' % D.HEAD_MAX_ROWS in hdr
    assert 'constexpr int kMmdMaxSigmas = %d;' % D.MMD_MAX_SIGMAS in text and 'ns > kMmdMaxSigmas || m + n > %d' % D.MMD_MAX_ROWS in text
    assert '__shared__ float cf[%d];' % D.MMD_MAX_ROWS in text and '__shared__ float gs_[GGAN_HEAD_BCE_MAX_ROWS];' in text
    assert 'd > %d || nx > %d' % (D.AGG_MAX, D.AGG_MAX) in text
    assert 'kind < 0 || kind > 2' in text and '(p == 1 || p == 2)' in text and 'if (unbiased && (m < 2 || n < 2)) return -1;' in text
    assert '#define GGAN_LOG2PI 1.8378770664093453f' in text and D.LOG2PI32 == np.float32(np.log(2 * np.pi))
    pw = _read('graphical_gan_amd', 'csrc', 'pointwise.h')
    assert 'constexpr int kBlock = %d;' % D.K_BLOCK in pw and '(size_t)kBlock * per_thread' in pw and 'int per_thread = 4' in pw
    assert 'if (b > %d) b = %d;' % (D.GRID_CAP, D.GRID_CAP) in pw
    # block sizes: every launch of losses.hip uses 256 but these
    blocks = {}
    for s in _LAUNCH.finditer(text):
        blocks.setdefault(s.group(5), set()).add(s.group(3))
    assert blocks == {'256': blocks['256'], '1024': {'dist_fwd_k'}, 'kBlock': {'dist_bwd_k'}, '64': {'mmd2_final_k', 'agg_div_final_k'},
                      '128': {'agg_div_fwd_k', 'agg_div_bwd_samples_k', 'agg_div_bwd_comps_k'}}, blocks
    assert (D.DIST_FWD_BLOCK, D.FINAL_BLOCK, D.AGG_BLOCK) == (1024, 64, 128)
    head = _read('graphical_gan_amd', 'csrc', 'cost_head.h')
    assert 'for (int r = rg; r < M; r += %d)' % D.HEAD_COLS in head and 'wg += cdiv(d.H, %d);' % D.HEAD_COLS in text
    build = _read('graphical_gan_amd', 'build.py')
    assert "'-ffp-contract=on'" in build and 'fast-math' not in build                        # what the rounding counts assume


def test_recorded_launches_follow_the_dispatch():
    for r in ROWS:
        assert D.planned(r) == r['launches'], (row_id(r), D.planned(r), r['launches'])
        assert all(len(l) == 5 and l[1] >= 1 for l in r['launches']) and r['note']
        assert len({(l[0], D.threads(l)) for l in r['launches']}) == len(r['launches'])     # what a profiler record can tell apart
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


# ---- the edges, from the rows ---------------------------------------------------------------------------------------------------------------
def _loop_strides(text):
    """-> {kernel: strides of its strided loops, as written}"""
    out = {}
    for m in re.finditer(r'__global__[^;{]*?void\s+(\w+)\((.*?)\n}\n', text, flags=re.S):
        out[m.group(1)] = sorted(set(re.findall(r'\+= ((?:\(size_t\))?(?:gridDim\.x \* )?blockDim\.x|256|128)\)', m.group(2))))
    return out


def test_rows_reach_a_second_trip_of_every_strided_loop():
    strides = _loop_strides(_source())
    assert strides['mmd2_rows_k'] == ['256'] and strides['mmd2_bwd_k'] == ['256'] and strides['gp_pen_k'] == ['blockDim.x']
    assert strides['agg_div_fwd_k'] == ['blockDim.x'] and strides['dist_fwd_k'] == ['blockDim.x'] and strides['bce_fwd_k'] == ['blockDim.x']
    # the grid-stride loops of the elementwise backward kernels never take a second trip: their grids cover n (grid_for caps at 2048 x 1024)
    assert strides['dist_bwd_k'] == ['(size_t)gridDim.x * blockDim.x'] and strides['bce_bwd_k'] == ['gridDim.x * blockDim.x']
    cost_head = _read('graphical_gan_amd', 'csrc', 'cost_head.h')
    assert 'for (int i = threadIdx.x; i < n; i += stride)' in cost_head
    of = lambda e, **kw: [r for r in ROWS if r['entry'] == e and all(r[k] == v for k, v in kw.items())]
    for kind in ('bce', 'mean'):
        assert {r['n'] for r in of('single', kind=kind)} == {1, 255, 256, 257, 800}                       # bce_fwd_k, mean_fwd_k: 256
        assert any(max(t[0] for t in r['terms']) > 256 for r in of('table', kind=kind))                   # cost_add_term: 256
        assert {len(r['terms']) for r in of('table', kind=kind)} == {1, 3, D.BCE_MAX}
        assert {t[0] for r in of('table', kind=kind) for t in r['terms']} == {1, 7, 256, 257, 800}
        assert {t[1] for r in of('table', kind=kind) for t in r['terms']} == {0.0, 1.0, 0.9}
        # idle workgroups of bce_multi_bwd_k's (cdiv(mx, 256), count) grid: a term shorter than the longest by more than a workgroup
        assert any(min(t[0] for t in r['terms']) + 256 <= max(t[0] for t in r['terms']) for r in of('table', kind=kind))
    assert any(n > 256 for r in of('heads') for _, _, ns in r['heads'] for n in ns)                       # the g loop of bce_head_bwd_k: 256
    for p in (1, 2):
        assert {r['n'] for r in of('dist', p=p)} == {1, 1023, 1024, 1025, 5000}                           # dist_fwd_k: 1024
    assert {(r['B'], r['D']) for r in of('gp')} == {(1, 1), (7, 255), (256, 256), (257, 257), (300, 5), (64, 3072)}
    assert any(r['D'] > 256 for r in of('gp')) and any(r['B'] > 256 for r in of('gp'))                    # gp_slopes_k / gp_fwd_grad_k, gp_pen_k
    for unb in (0, 1):
        assert any(r['m'] + r['n'] > 256 for r in of('mmd', unbiased=unb)) and any(r['d'] > 256 for r in of('mmd', unbiased=unb))
        assert any(r['m'] + r['n'] == D.MMD_MAX_ROWS for r in of('mmd', unbiased=unb))
    for kind in (0, 1, 2):
        assert {(r['nx'], r['nz'], r['d']) for r in of('agg', kind=kind, wide=False)} == \
            {(1, 1, 1), (5, 7, 3), (129, 3, 2), (4, 3, 129), (2, 2, D.AGG_MAX), (D.AGG_MAX, 2, 2)}      # dd += 128, j += 128, the limits
        assert any(r['n_coms'] != r['nx'] for r in of('agg', kind=kind))
    assert {r['kind'] for r in of('agg', wide=True)} == {0, 2}


def test_rows_reach_every_limit_optional_pointer_and_head():
    of = lambda e: [r for r in ROWS if r['entry'] == e]
    singles = of('single')
    assert {r['acc'] for r in singles} == {0, 1} and any(r['gloss'] != 1 for r in singles) and any(r['w'] != 1 for r in singles)
    heads = of('heads')
    assert {(M, H) for r in heads if len(r['heads']) == 1 for M, H, _ in r['heads']} == {(2, 1), (15, 16), (17, 17), (128, 33), (D.HEAD_MAX_ROWS, 5)}
    assert {len(ns) for r in heads if len(r['heads']) == 1 for _, _, ns in r['heads']} >= {1, 2, 4}
    two = [r for r in heads if len(r['heads']) == D.BCE_HEADS]
    assert two and any(r['heads'][0][:2] != r['heads'][1][:2] and [len(h[2]) for h in r['heads']] == [2, 2] for r in two)
    assert {r['dw'] for r in heads} == {True, False} and {r['db'] for r in heads} == {True, False} and all(r['alpha'] == 0.2 for r in heads)
    assert all(sum(ns) == M for r in heads for M, _, ns in r['heads'])
    for r in heads:
        assert all(np.any(h == 0) for h in _inp(ROWS.index(r))['h'])
    dist = of('dist')
    for p in (1, 2):
        assert {(r['gx'], r['gy']) for r in dist if r['p'] == p} == {(True, True), (False, True), (True, False)}
        assert {r['acc'] for r in dist if r['p'] == p} == {0, 1}
    mmd = of('mmd')
    assert {r['ns'] for r in mmd} == {1, 6, D.MMD_MAX_SIGMAS} and {r['wts'] for r in mmd} == {True, False}
    assert {(r['dX'], r['dY']) for r in mmd} == {(True, True), (False, True), (True, False)}
    assert {r['variant'] for r in mmd} == {'normal', 'shared', 'far'} and all(r['gout'] == 3.0 for r in mmd)
    assert (1, 1, 1, 0) in {(r['m'], r['n'], r['d'], r['unbiased']) for r in mmd} and not any(r['unbiased'] and min(r['m'], r['n']) < 2 for r in mmd)
    assert all(r['m'] + r['n'] <= D.MMD_MAX_ROWS for r in mmd) and all(max(r['nx'], r['d']) <= D.AGG_MAX for r in of('agg'))
    assert all(len(D.all_terms(r)) <= D.BCE_MAX for r in ROWS if r['entry'] in ('table', 'heads'))


def test_inputs_are_what_the_rows_promise():
    for i, r in enumerate(ROWS):
        inp = _inp(i)
        flat = np.concatenate([np.ravel(a) for v in inp.values() for a in (v if isinstance(v, list) else [v]) if a is not None])
        assert flat.dtype == np.float32 and np.all(np.isfinite(flat))
        assert not np.any((flat != 0) & (np.abs(flat) < D.TINY)), row_id(r)                  # no denormal goes in
        if r['entry'] == 'dist':
            same = inp['x'].view(np.uint32) == inp['y'].view(np.uint32)
            assert (same.any() and not same.all()) or r['n'] == 1
        if r['entry'] == 'gp':
            n = np.sqrt((inp['g'].astype(np.float64) ** 2).sum(1))
            assert np.sum(n == 1.0) >= 1 and n.min() >= 0.99e-3 and n.max() <= 30.1 and (r['B'] < 3 or (n.min() < 2e-3 and n.max() > 29))
        if r['entry'] == 'mmd' and r['variant'] == 'shared':
            assert np.array_equal(inp['X'][:2].view(np.uint32), inp['Y'][:2].view(np.uint32))
        if r['entry'] == 'mmd' and r['variant'] == 'far':
            assert np.all(np.abs(inp['Y'] - 200.0) < 10) and np.all(np.abs(inp['X']) < 10)     # every cross kernel underflows to 0
        if r['entry'] == 'agg' and r['wide']:
            assert np.all(inp['sd'] == 50.0)
    bce = [a for i, r in enumerate(ROWS) if r['entry'] == 'single' and r['kind'] == 'bce' and r['n'] >= 255 for a in [_inp(i)['x']]]
    for x in bce:
        assert set(np.asarray(D.EDGE_LOGITS, np.float32).view(np.uint32)) <= set(x.view(np.uint32))      # (+0 and -0 apart)


# ---- the bounds: not too tight for the right kernel, too tight for each wrong one -----------------------------------------------------------
@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_the_float32_restatement_passes_every_bound(idx):
    row, inp = ROWS[idx], _inp(idx)
    fr, broken = D.check(row, inp, D.run32(row, inp))
    print('COST %s (float32 numpy) fractions of the bound: %s' % (row_id(row), ' '.join('%s %.4f' % kv for kv in sorted(fr.items()))))
    assert not broken and D.within(fr) and set(fr) <= set(D.kernels_of(row)), (fr, broken)


# the row on which each wrong kernel is shown to miss
MUTANT_ROW = {
    'one_trip:cost': 'single-bce-n257-acc1', 'one_trip:heads_g': 'heads-2048x5t2', 'one_trip:dist': 'dist-p2-n1025-nogy-acc1',
    'one_trip:gp_slopes': 'gp-257x257', 'one_trip:gp_pen': 'gp-257x257', 'one_trip:mmd_rows': 'mmd-128-129-5-s1-wts-nodY-normal',
    'one_trip:mmd_bwd_j': 'mmdu-300-212-16-s8-wts-normal', 'one_trip:mmd_bwd_k': 'mmd-3-4-260-s6-wts-normal', 'one_trip:agg_d': 'agg-k0-4-3-129-c4',
    'one_trip:agg_nx': 'agg-k2-129-3-2-c129', 'accumulate_ignored': 'single-mean-n255-acc1', 'accumulate_always': 'single-bce-n1-acc0',
    'term0_added_to_stale': 'table-bce-c3-256_257_7', 'bce_no_abs': 'single-bce-n800-acc0', 'sigmoid_exp_ratio': 'single-bce-n255-acc1',
    'label_weight_swapped': 'table-bce-c3-256_257_7', 'n_from_longest': 'table-mean-c3-7_800_1', 'head1_reads_head0_terms': 'heads-17x17t2+40x33t2',
    'dbout_every_wg': 'heads-128x33t4', 'alpha_on_ge': 'heads-15x16t1-nodw', 'p1_plus_at_zero': 'dist-p1-n1023-nogy-acc0', 'gp_no_over_B': 'gp-300x5',
    'pen_stale_slope': 'gp-64x3072', 'unbiased_m2': 'mmdu-5-9-16-s8-nodX-normal', 'diagonal_kept': 'mmdu-256-256-8-s6-shared',
    'cross_plus': 'mmd-1-1-1-s1-normal', 'wts_ignored': 'mmdu-2-2-3-s6-wts-shared', 'gamma_no_half': 'mmd-5-9-16-s6-far',
    'jsd_shared_shift': 'agg-k2-6-9-40-c6-wide', 'ncoms_is_nx': 'agg-k2-5-7-3-c11', 'lognx_dropped': 'agg-k1-5-7-3-c5', 'gsd_no_inv_sg': 'agg-k2-1-1-1-c1',
}


@pytest.mark.parametrize('mut', D.MUTANTS)
def test_each_wrong_kernel_misses_on_its_row(mut):
    assert set(MUTANT_ROW) == set(D.MUTANTS)
    idx = _index(MUTANT_ROW[mut])
    row, inp = ROWS[idx], _inp(idx)
    fr, broken = D.check(row, inp, D.run32(row, inp, mut))
    print('COST wrong kernel %s on %s: worst fraction %.3g, broken %s' % (mut, row_id(row), max(fr.values()), broken))
    assert broken or max(fr.values()) > 2.0, (fr, broken)                        # by a margin, not by a rounding
    fr, broken = D.check(row, inp, D.run32(row, inp, None))
    assert not broken and D.within(fr)


def test_a_nan_or_a_touched_stage_in_any_output_fails():
    for rid, key in (('single-bce-n257-acc1', 'gx'), ('dist-p2-n1025-nogy-acc1', 'gx'), ('gp-7x255', 'gg'), ('mmd-5-9-16-s8-nodX-normal', 'dY'),
                     ('agg-k0-5-7-3-c5', 'gsd')):
        idx = _index(rid)
        row, inp = ROWS[idx], _inp(idx)
        out = D.run32(row, inp)
        out[key] = np.array(out[key], np.float32)
        out[key].flat[-1] = np.nan
        fr, broken = D.check(row, inp, out)
        assert broken and not D.within(fr), (rid, fr, broken)
    idx = _index('mmd-5-9-16-s8-nodX-normal')
    out = D.run32(ROWS[idx], _inp(idx))
    out['out'] = np.nextafter(np.float32(out['out']), np.float32(1))
    assert D.check(ROWS[idx], _inp(idx), out)[1]
    assert D._frac([1.0], [0.0]) == np.inf and D._frac([np.nan], [1.0]) == np.inf and D._frac([0.0], [0.0]) == 0.0
    assert not D.within({'a': float('nan')})


# ---- refused before any launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('item', D.REJECTED, ids=[r['id'] for r in D.REJECTED])
def test_rejected_calls_answer_before_any_launch(lib_built, item):
    """no device is needed: the answer comes before anything touches one, and the NaN-filled host buffers standing in for the outputs
    keep their bits"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    L.ggan_prof_reset()
    L.ggan_prof_enable(1)
    try:
        A = D.Alloc()
        rc = item['call'](L, A, None)
    finally:
        L.ggan_prof_enable(0)
    msg = (L.ggan_last_error() or b'').decode()
    assert rc != 0 and item['fn'] in msg, (rc, msg)
    assert _lib.prof_report() == [] and A.outs and A.outputs_untouched()
    L.ggan_prof_reset()


def test_the_rejected_list_is_the_issues():
    ids = ' '.join(r['id'] for r in D.REJECTED)
    for what in ('count0', 'count17', 'nheads3', 'M2049', 'terms-do-not-cover-rows', 'dist_fwd-p3', 'dist_bwd-p3', 'rows513', 'ns9', 'mmd2u_fwd-m1',
                 'mmd2u_bwd-m1', 'd8193', 'nx8193', 'kind3'):
        assert what in ids, what
