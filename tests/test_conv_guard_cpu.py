"""tests/_conv_guard.py on the CPU: its rows are well formed, the 'exact' data set stays below 2^23 on every row, every row of the
dispatch table and of EXTRA_ROWS runs with both data sets or is a stated exception, check() accepts a float32 numpy evaluation of every
op and rejects every mutant on its row -- and the `>=` and never-stored mutants pass what test_conv_dispatch_gpu.py checks today.  The
activation-derivative selects written out by hand in csrc/conv_*.hip, and the act_grad calls there, are read from the sources: each
belongs to a kernel that a masked row (LeakyReLU and ReLU) runs, so a new site without a row fails here."""
import os
import re

import numpy as np
import pytest

import _conv_guard as G
from _conv_dispatch import ROWS
from _conv_guard import EXTRA_ROWS, MISALIGNED, ALL_ROWS, guard_id
from test_conv_dispatch_cpu import CSRC, _read, family_names, launched_names, HELPERS

# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
OPS = {'fwd', 'fwd_masked', 'fwd_cast', 'dgrad', 'dgrad_masked', 'dgrad_bias_act', 'wgrad', 'wgrad_act', 'wgrad_parts'}
SWITCHES = {'GGAN_DG16', 'GGAN_DG16_FORCE', 'GGAN_DG16_KQ', 'GGAN_NO_THIN', 'GGAN_WGRAD_SPLIT', 'GGAN_WGRAD_W4', 'GGAN_FWD_SK', 'GGAN_DGRAD_SK',
            'GGAN_WGRAD_SK'}
OPERANDS = {'fwd': ('x', 'w'), 'dgrad': ('gy', 'w'), 'dgrad_masked': ('gy', 'w', 'yref'), 'wgrad': ('x', 'gy'), 'wgrad_act': ('x', 'gy', 'yref')}


def test_figures_are_those_of_the_ops_tests():
    import test_ops_gpu as T
    assert (G.TOL, G.TOL_LONG) == (T.TOL, T.TOL_LONG)
    with open(os.path.join(os.path.dirname(CSRC), '..', 'include', 'ggan.h')) as f:
        assert int(re.search(r'#define GGAN_WS_RESERVED (\d+)', f.read()).group(1)) == G.WS_RESERVED


def test_rows_are_well_formed():
    ids = [guard_id(r) for r in ALL_ROWS]
    assert len(set(ids)) == len(ids)
    names = family_names()
    helpers = set()
    for f in HELPERS:
        helpers |= launched_names(_read(f))
    for r in EXTRA_ROWS + MISALIGNED:
        assert r['op'] in OPS and set(r['env']) <= SWITCHES, r
        N, Ci, H, W, Co, pad = r['geom']
        assert pad == 'SAME' and N <= 16 and max(H, W) <= 132 and N * Ci * H * W * Co <= 2 ** 24, r
        assert r['tiles'] >= 1 and r['sk'] >= 1 and r['block'] in (256, 512, 1024) and r['target'] >= 0, r
        assert r['kernel'] in names and set(r['also']) <= names | helpers, r
        reduces = [a for a in r['also'] if a.startswith('splitk_reduce')]
        assert len(reduces) == (1 if r['sk'] > 1 and r['op'] != 'wgrad_parts' else 0), r
        assert ('plan' in r) == r['kernel'].startswith('corr_kernel<'), r
        if 'plan' in r:
            mode, wm, wn, ks, pw, x4 = r['kernel'][len('corr_kernel<'):-1].split(', ')
            assert r['op'].startswith('fwd') == (mode == '0') and r['plan']['xq'] == (4 if x4 == 'true' else 1), r
            assert r['block'] == 64 * int(wm) * int(wn) * int(ks), r
        assert not r.get('nobias') or r['op'] == 'wgrad_act', r
    assert all('off' not in r for r in EXTRA_ROWS)
    for r in ALL_ROWS:                       # a band holds a whole image plane: a halo row read in front of the tensor lands in it
        assert G.band(r) >= max(r['geom'][2] * r['geom'][3], 1024) and G.band(r) % 4 == 0, r
        segs = G.ws_segments(r)
        assert all(a + n <= G.WS_FLOATS for a, n in segs), (r, segs)
        if 'pad_width_k' in r['also']:       # the widened path wants 1 MiB behind its copies (conv_api.hip: wgrad_widened)
            assert 4 * (segs[1][0] + segs[1][1] + 64) + (1 << 20) <= 4 * G.WS_FLOATS, r


def test_extra_rows_keep_the_non_square_cases():
    hw = lambda pred: {tuple(r['geom'][2:4]) for r in EXTRA_ROWS if pred(r)}
    corr = lambda mode: (lambda r: r['kernel'].startswith('corr_kernel<%d' % mode))
    assert {(8, 16), (16, 8)} <= hw(corr(0)) and {(8, 16), (16, 8)} <= hw(corr(1)) and {(8, 16), (16, 8)} <= hw(corr(2))
    for geom in ((7, 8), (8, 28)):           # pad_t != pad_l, on every kind of op
        ops = {r['op'] for r in EXTRA_ROWS if tuple(r['geom'][2:4]) == geom}
        assert {'fwd', 'dgrad', 'dgrad_masked', 'wgrad', 'wgrad_act'} <= ops, (geom, ops)
    assert G.same_pads(7) == (4, 2) and G.same_pads(8) == (4, 1) and G.same_pads(28) == (14, 1)
    for k in ('thin_fwd_kernel', 'thin_dgrad_kernel', 'thin_wgrad_kernel'):
        assert {(16, 32), (32, 16)} <= hw(lambda r: r['kernel'] == k and r['geom'][1] <= 4), k
    assert {(8, 16), (16, 8)} <= hw(lambda r: r['kernel'].startswith('wgrad_kernel<') and not r['also'])
    for r in EXTRA_ROWS:                     # non-square rows cover each op plain and masked / with the bias sum
        if r['geom'][2] != r['geom'][3] and r['op'] in ('dgrad', 'wgrad') and r['kernel'] != 'conv_wgrad_naive':
            twin = 'dgrad_masked' if r['op'] == 'dgrad' else 'wgrad_act'
            assert any(t['op'] == twin and t['geom'] == r['geom'] for t in EXTRA_ROWS), r


def test_misaligned_rows_name_every_operand_with_a_host_predicate():
    """one row per operand and path: forward and thin forward (x, w), data gradient, dg16 and thin data gradient (gy, w, the mask
    reference), filter gradient and thin filter gradient (x, gy, the mask reference)"""
    for r in MISALIGNED:
        assert r['off'] in OPERANDS[r['op']], r
        aligned = [a for a in ROWS if a['op'] == r['op'] and a['geom'] == r['geom'] and a['env'] == r['env'] and a['target'] == r['target']]
        assert all(a['kernel'] != r['kernel'] or r['also'] != a['also'] for a in aligned), (r, aligned)       # ... and another kernel runs
    paths = {}
    for r in MISALIGNED:
        key = (r['geom'], tuple(sorted(r['env'].items())))
        paths.setdefault(key, set()).add(r['off'])
    want = sorted([('w', 'x')] * 2 + [('gy', 'w', 'yref')] * 3 + [('gy', 'x', 'yref')] * 2)
    assert sorted(tuple(sorted(v)) for v in paths.values()) == want, paths


def test_exact_data_stays_exact_in_float32():
    for r in ALL_ROWS:
        assert G.exact_bound(r) < 2 ** 23, r
        if 'exact' not in G.data_sets(r):
            continue
        for m in G.masks(r):
            inp = G.inputs(r, 'exact', m)
            assert inp['alpha'] == 0.5
            for k, lim in (('x', 2), ('gy', 2), ('w', 1), ('b_o', 3), ('b_i', 3)):
                assert np.all(inp[k] == np.round(inp[k])) and np.abs(inp[k]).max() <= lim, (r, k)


def test_every_row_runs_both_data_sets_or_is_a_stated_exception():
    left_out = [r for r in ROWS + EXTRA_ROWS if G.data_sets(r) != ('gauss', 'exact')]
    assert [(r['kernel'], r['op']) for r in left_out] == [('thin_fwd_kernel', 'fwd_cast')]
    assert all(G.data_sets(r) == ('gauss',) for r in left_out)
    for r in ALL_ROWS:
        assert G.masks(r) == (('lrelu', 'relu') if r['op'] in G.MASKED_OPS else (None,)), r
    import test_conv_guard_gpu as T
    assert [(guard_id(r), d) for r, d in T.CASES] == [(guard_id(r), d) for r in ROWS + EXTRA_ROWS + MISALIGNED for d in G.data_sets(r)]


def test_mask_reference_has_exact_zeros_of_both_signs():
    for r in ALL_ROWS:
        if r['op'] not in G.MASKED_OPS:
            continue
        ref = G.inputs(r, 'gauss', 'relu')['yref']
        zeros = ref == 0.0
        assert abs(int(zeros.sum()) - ref.size // 10) <= 1 and ref.size >= 20, r
        neg = int(np.signbit(ref[zeros]).sum())
        assert abs(2 * neg - int(zeros.sum())) <= 1, r
        inp = G.inputs(r, 'gauss', 'lrelu')
        assert np.all(G.slope(inp)[inp['yref'] == 0.0] == 0.2) and np.all(G.slope(dict(inp, mask='relu'))[inp['yref'] == 0.0] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# check(): accepts a correct run of every row, rejects every mutant
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('data', ['gauss', 'exact'])
def test_check_accepts_a_float32_evaluation_of_every_row(data):
    n = 0
    for r in ALL_ROWS:
        if data not in G.data_sets(r):
            continue
        for m in G.masks(r):
            bufs, recs = G.simulate(r, data, m)
            errs = G.check(r, data, bufs, recs)
            assert errs and all(e < 2e-7 for e in errs.values()), (r, errs)        # (float64 -> float32: half an ulp of the largest value)
            n += 1
    assert n >= len(ALL_ROWS) - 1


def _rejects(row, data, bufs, recs):
    try:
        G.check(row, data, bufs, recs)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize('name', sorted(G.MUTANTS))
def test_check_rejects_the_mutant_on_its_row(name):
    assert sorted(G.MUTANTS) == sorted(G.MUTANT_ROW)
    row, data, bufs, recs = G.mutant(name)
    mask = G.MUTANTS[name][2]
    ok_bufs, ok_recs = G.simulate(row, data, mask)
    assert _rejects(row, data, ok_bufs, ok_recs) is None                          # the same row, unharmed, passes
    why = _rejects(row, data, bufs, recs)
    print(name, guard_id(row), why)
    assert why is not None, name
    expect = dict(store_behind_output='a store behind the output', quad_never_stored='4 elements nobody stored',
                  nan_through_top_halo='1 elements nobody stored', unwritten_slab_added='elements nobody stored',
                  slab_counted_twice='elements differ')
    if name in expect:
        assert expect[name] in why, (name, why)
    if name == 'pads_swapped':
        assert tuple(row['geom'][2:4]) == (7, 8)
    if name in ('unwritten_slab_added', 'slab_counted_twice'):
        assert row['sk'] > 1
    if name == 'quad_never_stored':                                                # ragged image group
        assert row['geom'][0] % row['plan']['tile'][0] != 0


def test_unwritten_workspace_and_wrong_slab_count_are_seen():
    row = G.find_row('fwd', (2, 64, 8, 8, 32))
    head = G.WS_RESERVED // 4
    bufs, recs = G.simulate(row, 'gauss')
    bufs['ws'][head + G.out_elems(row)] = np.nan                                   # second slab: one float never written
    assert 'never written' in _rejects(row, 'gauss', bufs, recs)
    bufs, recs = G.simulate(row, 'gauss')
    bufs['ws'][head + 2 * G.out_elems(row)] = 0.0                                  # a third slab
    assert 'outside the row' in _rejects(row, 'gauss', bufs, recs)
    bufs, recs = G.simulate(row, 'gauss')
    bufs['ws'][7] = 1.0                                                            # an arrival counter left behind
    assert 'reserved head' in _rejects(row, 'gauss', bufs, recs)
    one = G.find_row('fwd', (3, 6, 16, 16, 20))                                    # sk == 1: nothing behind the head is finite
    bufs, recs = G.simulate(one, 'gauss')
    bufs['ws'][head] = 0.0
    assert 'outside the row' in _rejects(one, 'gauss', bufs, recs)
    parts = [r for r in ROWS if r['op'] == 'wgrad_parts' and r['sk'] > 1][0]       # the bias tail of a slab is checked like the slab
    bufs, recs = G.simulate(parts, 'exact', 'relu')
    whole, off, cap = bufs['part']
    whole[off + 2 * recs['stride'] - 1] = np.nan
    assert 'never written' in _rejects(parts, 'exact', bufs, recs)
    bufs, recs = G.simulate(parts, 'exact', 'relu')
    whole, off, cap = bufs['part']
    whole[off + recs['stride'] - 1] += 1.0
    assert 'slabs_gb' in _rejects(parts, 'exact', bufs, recs)


@pytest.mark.parametrize('mask', ['lrelu', 'relu'])
def test_the_present_check_passes_the_ge_mutant(mask):
    """test_conv_dispatch_gpu.py draws a continuous mask reference and asserts it has no zero: there `>=` and `>` are the same function"""
    name = 'mask_ge_' + mask
    row = G.find_row(*G.MUTANT_ROW[name])
    rng = np.random.default_rng(5)
    N, Ci, H, W, Co, _ = row['geom']
    yref = rng.standard_normal((N, Co) + G.out_hw(row)).astype(np.float32)
    assert np.all(yref != 0.0)
    got, ref = G.ge_result(row, 'gauss', mask, yref=yref)
    assert G.present_check(row, got, ref)
    got, ref = G.ge_result(row, 'gauss', mask)                                     # ... and with the zeros of this module it does not
    assert not G.present_check(row, got, ref)


def test_the_present_check_passes_the_never_stored_mutant():
    """an output from torch.empty can be a block an earlier test left the right values in: the quad nobody stores is then right"""
    row = G.find_row(*G.MUTANT_ROW['quad_never_stored'])
    bufs, recs, quad = G._never_stored_result(row, 'gauss', None)                 # the buffer held the right values beforehand
    whole, off, shape = bufs['out']['y']
    got = dict(y=whole[off:off + int(np.prod(shape))].reshape(shape))
    assert G.present_check(row, got, recs['ref'])
    whole[quad] = np.nan                                                           # here it held NaN
    assert 'nobody stored' in _rejects(row, 'gauss', bufs, recs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the activation-derivative sites of the sources
# ---------------------------------------------------------------------------------------------------------------------------------
SITE_FILES = ('conv_corr.hip', 'conv_dg16.hip', 'conv_thin.hip', 'conv_wgrad.hip', 'conv_wgrad_split.hip', 'conv_naive.hip', 'conv_api.hip')
_SELECT = re.compile(r'> 0\.f \?')
_ACT_GRAD = re.compile(r'\bact_grad\(')
_FUNC = re.compile(r'^(?:template\s*<[^>]*>\s*)?(?:__global__|__device__|static)\b[^;{}]*?\bvoid\s+(\w+)\s*\(', re.M)

# (file, enclosing function, kind of site) -> what a row must be to run it
SITES = {
    ('conv_corr.hip', 'corr_body', 'select'): [lambda r: r['kernel'].startswith('corr_kernel<1') and r['op'] == 'dgrad_masked',
                                               lambda r: r['kernel'].startswith('corr_kernel<2') and r['op'] == 'dgrad_masked',
                                               lambda r: r['kernel'].endswith('true>') and r['op'] == 'dgrad_masked',       # the 16-byte units
                                               lambda r: r['kernel'].endswith('false>') and r['op'] == 'dgrad_masked'],
    ('conv_corr.hip', 'corr_body', 'act_grad'): [lambda r: r['kernel'].startswith('corr_kernel<0') and r['kernel'].endswith('true>') and r['op'] == 'fwd_masked',
                                                 lambda r: r['kernel'].startswith('corr_kernel<0') and r['kernel'].endswith('false>') and r['op'] == 'fwd_masked'],
    ('conv_dg16.hip', 'dg16_body', 'select'): [lambda r: r['kernel'].startswith('dg16_kernel<') and r['op'] == 'dgrad_masked'],
    ('conv_thin.hip', 'thin_dgrad_kernel', 'select'): [lambda r: r['kernel'] == 'thin_dgrad_kernel' and r['op'] == 'dgrad_masked'],
    ('conv_thin.hip', 'thin_wgrad_kernel', 'select'): [lambda r: r['kernel'] == 'thin_wgrad_kernel' and r['op'] == 'wgrad_act',
                                                       lambda r: r['kernel'] == 'thin_wgrad_kernel' and r['op'] == 'wgrad_parts'],
    ('conv_thin.hip', 'thin_fwd_kernel', 'act_grad'): [lambda r: r['kernel'] == 'thin_fwd_kernel' and r['op'] == 'fwd_masked'],
    ('conv_wgrad.hip', 'wgrad_kernel', 'select'): [lambda r: r['kernel'].startswith('wgrad_kernel<') and r['op'] == 'wgrad_act',
                                                   lambda r: r['kernel'].startswith('wgrad_kernel<') and r['op'] == 'wgrad_parts'],
    ('conv_wgrad.hip', 'wgrad4_kernel', 'select'): [lambda r: r['kernel'].startswith('wgrad4_kernel<') and r['kernel'].endswith(', true>') and r['op'] == 'wgrad_act',
                                                    lambda r: r['kernel'].startswith('wgrad4_kernel<') and not r['kernel'].endswith(', true>') and r['op'] == 'wgrad_act'],
    ('conv_naive.hip', 'conv_dgrad_naive_k', 'act_grad'): [lambda r: r['kernel'] == 'conv_dgrad_naive' and r['op'] == 'dgrad_masked'],
    ('conv_naive.hip', 'conv_wgrad_naive_k', 'act_grad'): [lambda r: r['kernel'] == 'conv_wgrad_naive' and r['op'] == 'wgrad_act'],
    ('conv_api.hip', 'pad_width_k', 'act_grad'): [lambda r: 'pad_width_k' in r['also'] and r['op'] == 'wgrad_act'],
}


def sites(csrc=CSRC):
    """-> {(file, enclosing function, 'select' | 'act_grad'): [line numbers]} of every `ref > 0.f ? v : v * slope` select written out by
    hand and every act_grad call in the conv2d sources, comments left out"""
    out = {}
    for name in SITE_FILES:
        text = _read(name, csrc)
        funcs = [(m.start(), m.group(1)) for m in _FUNC.finditer(text)]
        pos = 0
        for no, line in enumerate(text.split('\n'), 1):
            code = line.split('//')[0]
            for kind, rx in (('select', _SELECT), ('act_grad', _ACT_GRAD)):
                if rx.search(code):
                    before = [f for p, f in funcs if p <= pos]
                    assert before, (name, no, line)
                    out.setdefault((name, before[-1], kind), []).append(no)
            pos += len(line) + 1
    return out


def uncovered_sites(csrc=CSRC):
    found = sites(csrc)
    rows = ROWS + EXTRA_ROWS
    unknown = sorted(k for k in found if k not in SITES)
    stale = sorted(k for k in SITES if k not in found)
    unrun = sorted((k, i) for k, preds in SITES.items() for i, p in enumerate(preds) if not any(p(r) for r in rows))
    return unknown, stale, unrun


def test_every_activation_derivative_site_belongs_to_a_kernel_a_masked_row_runs():
    found = sites()
    print({k: v for k, v in found.items()})
    assert sum(len(v) for k, v in found.items() if k[2] == 'select') >= 24 and sum(len(v) for k, v in found.items() if k[2] == 'act_grad') >= 8
    unknown, stale, unrun = uncovered_sites()
    assert not unknown, 'activation-derivative sites in functions tests/test_conv_guard_cpu.py SITES does not know: %s' % unknown
    assert not stale, 'SITES names functions that hold no site any more: %s' % stale
    assert not unrun, 'no masked row of ROWS + EXTRA_ROWS runs %s' % unrun
    for r in ROWS + EXTRA_ROWS:                  # and a masked row runs LeakyReLU and ReLU
        if any(p(r) for preds in SITES.values() for p in preds):
            assert G.masks(r) == ('lrelu', 'relu'), r


def test_a_scratch_copy_with_a_new_site_is_caught(tmp_path):
    for f in SITE_FILES:
        text = _read(f)
        if f == 'conv_dg16.hip':
            text += ('\ntemplate <int K>\n__global__ void dg16_tail_kernel(const float* g, const float* ref, float* o, float slope) {\n'
                     '    const float v = g[threadIdx.x];\n    o[threadIdx.x] = ref[threadIdx.x] > 0.f ? v : v * slope;\n}\n')
        if f == 'conv_naive.hip':
            text = text.replace('act_grad(', 'act_deriv(')
        (tmp_path / f).write_text(text)
    unknown, stale, unrun = uncovered_sites(str(tmp_path))
    assert unknown == [('conv_dg16.hip', 'dg16_tail_kernel', 'select')], unknown
    assert stale == [('conv_naive.hip', 'conv_dgrad_naive_k', 'act_grad'), ('conv_naive.hip', 'conv_wgrad_naive_k', 'act_grad')], stale
