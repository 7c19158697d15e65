"""The coverage table tests/_optim_dispatch.py against csrc/optim.hip, without a GPU: the GGAN_LAUNCH sites of the five optimizer
entry points have rows and the rows name no other label; the constants planned() copies are the source's; every row's launches follow
from planned(); the table reaches every (path, chunk, tail) combination and every arrival-group case; the float64 restatement agrees
with oracle.ops.adam_update; a float32 restatement of the kernels passes every bound while each of sixteen wrong kernels misses one by
more than a factor of two; and the argument checks of the entry points answer before any launch."""
import ctypes as C
import os
import re

import numpy as np

import _optim_dispatch as D
from _optim_dispatch import ROWS, row_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'ggan_pack_parts2': 'pack', 'ggan_pack_adam': 'pack_adam', 'ggan_adam_step': 'adam_step', 'ggan_adam_step_counted': 'adam_step',
                'ggan_adam_advance': 'adam_advance', 'ggan_rmsprop_step': 'rmsprop_step'}
SMALL = 100000                  # rows with more elements are left to the GPU module (the power of the inputs does not grow with n)


def _source():
    text = ''
    for name in ('optim.hip', 'pointwise.h'):           # the optimizer's unit, then kBlock and grid_for, which it shares
        with open(os.path.join(ROOT, 'graphical_gan_amd', 'csrc', name)) as f:
            text += f.read()
    return text


def _elements(row):
    return row['n'] if row['n'] else sum(t['size'] for t in row['tensors'])


# ---- launch sites against rows ---------------------------------------------------------------------------------------------------------------
_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*,\s*[^,]+,\s*[^,]+,\s*(\w+)(?:<([^()<>]*)>)?\s*,')


def entry_sites(text):
    """-> {entry point: [(label, kernel, template argument or None)]} of the GGAN_LAUNCH sites inside the bodies of ENTRY_POINTS"""
    out = {}
    for name in ENTRY_POINTS:
        m = re.search(r'^int %s\(' % name, text, flags=re.M)
        assert m, name
        body = text[m.start():text.index('\n}\n', m.start())]
        out[name] = [(s.group(1), s.group(2), s.group(3)) for s in _LAUNCH.finditer(body)]
        assert len(out[name]) == body.count('GGAN_LAUNCH('), name
    return out


def uncovered(text, rows=ROWS):
    """-> (labels of the entry points' sites no row names, labels rows name that no site has)"""
    sites = {s[0] for v in entry_sites(text).values() for s in v}
    named = {l[0] for r in rows for l in r['launches']}
    return sorted(sites - named), sorted(named - sites)


def test_every_site_has_a_row_and_every_row_a_site():
    text = _source()
    sites = entry_sites(text)
    assert {k: [s[0] for s in v] for k, v in sites.items()} == {k: [v] for k, v in ENTRY_POINTS.items()}
    assert uncovered(text) == ([], [])
    # adam_k<false> and adam_k<true> share the label: the rows tell them apart by entry point, and both have rows
    assert sites['ggan_adam_step'] == [('adam_step', 'adam_k', 'false')] and sites['ggan_adam_step_counted'] == [('adam_step', 'adam_k', 'true')]
    assert {'adam_step', 'adam_step_counted', 'pack', 'pack_adam', 'rmsprop_step'} == {r['entry'] for r in ROWS}
    assert sites['ggan_pack_adam'][0][1] == 'pack_adam_k' and sites['ggan_pack_parts2'][0][1] == 'pack_k'
    assert sites['ggan_rmsprop_step'][0][1] == 'rmsprop_k'


def test_a_scratch_copy_with_a_new_or_a_lost_site_is_caught():
    text = _source()
    site = 'GGAN_LAUNCH("rmsprop_step"'
    assert text.count(site) == 1
    assert uncovered(text.replace(site, 'GGAN_LAUNCH("rmsprop_centered"')) == (['rmsprop_centered'], ['rmsprop_step'])
    assert uncovered(text, [r for r in ROWS if r['entry'] != 'pack']) == (['pack'], [])


# ---- constants and the plan ------------------------------------------------------------------------------------------------------------------
def test_transcribed_constants_are_the_sources():
    text = _source()
    assert 'constexpr int kBlock = %d;' % D.K_BLOCK in text and 'constexpr int kPackChunk = %d;' % D.PACK_CHUNK in text
    assert 'pack_chunk(int slabs) { return slabs > %d ? %d : kPackChunk; }' % (D.PACK_SLABS_MANY, D.PACK_CHUNK_MANY) in text
    assert 'if (b > %d) b = %d;' % (D.GRID_CAP, D.GRID_CAP) in text and 'if (b < 1) b = 1;' in text
    assert 'int gx = (int)cdivz(mx, (size_t)kBlock * 16);' in text and D.K_BLOCK * 16 == D.PACK_CHUNK
    assert 'if (gx > %d) gx = %d;' % (D.PACK_GRID_CAP, D.PACK_GRID_CAP) in text and 'if (gx < 1) gx = 1;' in text
    assert text.count('dim3(grid_for(n, %d)), dim3(kBlock)' % D.STEP_PER_THREAD) == 3          # adam_k<false>, adam_k<true>, rmsprop_k
    assert 'nb += (int)cdivz(sizes[i] > 0 ? sizes[i] : 1, (size_t)pack_chunk(t.parts[i] + (t.src2[i] ? t.parts2[i] : 0)));' in text
    pred = ('if (s && ((((uintptr_t)s) | ((uintptr_t)d) | ((uintptr_t)s2)) & 15) == 0 && (np == 1 || (ps & 3) == 0) && '
            '(np2 <= 1 || (ps2 & 3) == 0)) {')
    assert text.count(pred) == 2                                                             # pack_k and pack_adam_k
    assert 'if (base + chunk >= n && (n4 << 2) + threadIdx.x < n) one((n4 << 2) + threadIdx.x);' in text
    assert 'const int grp = blockIdx.x & %d, members = ((int)gridDim.x - grp + %d) >> 5, groups = gridDim.x < %d ? (int)gridDim.x : %d;' \
        % (D.ARRIVE_GROUPS - 1, D.ARRIVE_GROUPS - 1, D.ARRIVE_GROUPS, D.ARRIVE_GROUPS) in text
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert '#define GGAN_PACK_MAX %d' % D.PACK_MAX in hdr and '#define GGAN_PACK_ARRIVE_STRIDE %d' % D.ARRIVE_STRIDE in hdr
    assert '#define GGAN_PACK_ARRIVE_INTS (%d * GGAN_PACK_ARRIVE_STRIDE)' % (D.ARRIVE_GROUPS + 1) in hdr
    from graphical_gan_amd import _lib
    assert _lib.PACK_MAX == D.PACK_MAX and _lib.PACK_ARRIVE_INTS == D.ARRIVE_INTS == (D.ARRIVE_GROUPS + 1) * D.ARRIVE_STRIDE
    build = open(os.path.join(ROOT, 'graphical_gan_amd', 'build.py')).read()
    assert "'-ffp-contract=on'" in build and 'fast-math' not in build                        # what the rounding counts assume


def test_recorded_launches_follow_the_dispatch():
    for r in ROWS:
        assert D.planned(r) == r['launches'], (row_id(r), D.planned(r), r['launches'])


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    big = [r for r in ROWS if 4 * _elements(r) > 4 << 20]
    assert sorted(r['entry'] for r in big) == ['adam_step', 'adam_step_counted', 'pack', 'pack', 'rmsprop_step', 'rmsprop_step'], [row_id(r) for r in big]
    for r in ROWS:
        assert all(len(l) == 4 and l[1] >= 1 for l in r['launches']) and r['note'], r
        if r['entry'] in ('pack', 'pack_adam'):
            assert 0 < len(r['tensors']) <= D.PACK_MAX and not r['n'], row_id(r)
            offs, total = D.layout(r['tensors'])
            end = D.PAD
            for t, off in zip(r['tensors'], offs):
                assert off >= end + 4 and off % 4 == t['slot'] and t['parts'] >= 1, row_id(r)          # sentinels between the slots
                assert t['parts'] == 1 or t['stride'] >= t['size'], row_id(r)
                assert t['parts2'] <= 1 or t['stride2'] >= t['size'], row_id(r)
                end = off + t['size']
            assert end + D.PAD <= total
            assert not r['split'] or (r['entry'] == 'pack_adam' and 0 < r['split'] < len(r['tensors']) and r['repeat'] == 1), row_id(r)
        else:
            assert r['n'] > 0 and not r['tensors'] and r['repeat'] == 1, row_id(r)
        assert r['entry'] == 'rmsprop_step' or r['clip'] is None


def test_table_reaches_every_path_chunk_and_tail_combination():
    seen, sizes = set(), {}
    for r in ROWS:
        if r['entry'] != 'pack_adam':
            continue
        for lo, hi, _ in D.segments(r):
            for t, p in zip(r['tensors'][lo:hi], D.tensor_plans(r, lo, hi)):
                seen.add((p['path'], p['chunk'], p['tail'] is not None, p['tail_only']))
                sizes.setdefault((p['path'], p['chunk']), set()).add(t['size'])
                assert p['tail'] is None or p['tail'] == p['last']
                assert p['last'] - p['first'] + 1 == D.cdiv(max(t['size'], 1), p['chunk'])
    want = {('scalar', c, False, False) for c in (1024, 4096)} | {('float4', c, tail, only) for c in (1024, 4096)
                                                                  for tail, only in ((False, False), (True, False), (True, True))}
    assert seen == want, sorted(seen ^ want)
    for c in (1024, 4096):                       # a whole chunk, one float4 group and one element on each side of it, on both paths
        for path in ('float4', 'scalar'):
            assert {c - 1, c, c + 3} <= sizes[(path, c)] or {c - 1, c, c + 1} <= sizes[(path, c)], (path, c, sorted(sizes[(path, c)]))
    assert set(D.SIZES) <= sizes[('float4', 4096)] and set(D.SIZES) <= sizes[('scalar', 4096)]
    pa = [r for r in ROWS if r['entry'] == 'pack_adam']
    # a tail-only workgroup is what 4097 is there for; a missing source with and without src2; a size-0 tensor between two others
    assert any(t['size'] == 4097 and p['tail_only'] for r in pa for t, p in zip(r['tensors'], D.tensor_plans(r)))
    assert any(not t['src'] and not t['parts2'] for r in pa for t in r['tensors'])
    assert any(not t['src'] and t['parts2'] for r in pa for t in r['tensors'])
    assert any(r['tensors'][k]['size'] == 0 and 0 < k < len(r['tensors']) - 1 for r in pa for k in range(len(r['tensors'])))
    assert any(len(r['tensors']) == D.PACK_MAX and {t['size'] for t in r['tensors']} == set(range(1, 8)) for r in pa)
    assert any(r['split'] for r in pa)
    # the slab cases: both sides of pack_chunk's `> 4`, with and without src2; odd strides on either source; a src2 off its boundary
    slabs = {(t['parts'], t['parts2'], t['stride'] % 4, t['stride2'] % 4, t['soff2']) for r in pa for t in r['tensors']}
    assert {(2, 0, 0, 0, 0), (3, 0, 1, 0, 0), (4, 0, 0, 0, 0), (4, 1, 0, 0, 0), (5, 0, 0, 0, 0), (1, 4, 0, 0, 0), (1, 2, 0, 1, 0), (1, 1, 0, 0, 1)} <= slabs
    assert {r['step0'] for r in pa} >= {0, 1, 9, 999, 99999} and {r['hyper'] for r in pa} == {D.HP, D.HP99}
    assert {r['gscale'] for r in pa} == {1.0, 0.5, 1.0 / 3}
    # the same tables through ggan_pack_parts2, with and without the counter, and the capped grid
    pk = [r for r in ROWS if r['entry'] == 'pack']
    assert all(any(q['tensors'] == r['tensors'] for q in pk) for r in pa if r['repeat'] == 1 and not r['split'] and len(r['tensors']) > 2)
    assert {r['bump'] for r in pk} == {True, False} and any(r['bump'] and r['repeat'] > 1 for r in pk)
    assert any(max(t['size'] for t in r['tensors']) == D.PACK_GRID_CAP * D.PACK_CHUNK + 4099 and r['launches'][0][2][0] == D.PACK_GRID_CAP for r in pk)
    # adam_k / rmsprop_k
    for e in ('adam_step', 'adam_step_counted'):
        rows = [r for r in ROWS if r['entry'] == e]
        assert {r['n'] for r in rows} == {1, 3, 4, 5, 255, 1025, D.BIG} and {r['gscale'] for r in rows} == {1.0, 0.5, 1.0 / 3}, e
        assert {D.ordinal(r) for r in rows} == {1, 2, 10, 1000, 100000} and {r['hyper'] for r in rows} == {D.HP, D.HP99}, e
    assert D.BIG == 2048 * 256 * 8 + 1027 and D.cdiv(D.BIG, 2048) > D.GRID_CAP
    rms = [r for r in ROWS if r['entry'] == 'rmsprop_step']
    assert {(r['n'], r['clip']) for r in rms} == {(n, c) for n in (1, 5, 1025, D.BIG) for c in (None, D.CLIP)}
    assert {r['gscale'] for r in rms} == {1.0, 1.0 / 3} and {r['hyper'] for r in rms} == {(5e-5, 0.9, 1e-10)}


def test_table_reaches_the_arrival_group_cases():
    nbs = sorted({l[2][0] for r in ROWS if r['entry'] == 'pack_adam' and r['repeat'] == 3 for l in r['launches']})
    assert nbs == [1, 31, 32, 33, 64, 65]
    for r in ROWS:
        if r['entry'] == 'pack_adam' and r['repeat'] == 3:
            nb = r['launches'][0][2][0]
            assert r['tensors'][0]['size'] == (nb - 1) * D.PACK_CHUNK + 5 and r['launches'][0][1] == 3
    got = {nb: D.arrival_groups(nb) for nb in nbs}
    assert got[1] == (1, [1]) and got[31] == (31, [1] * 31) and got[32] == (32, [1] * 32)
    assert got[33] == (32, [2] + [1] * 31) and got[64] == (32, [2] * 32) and got[65] == (32, [3] + [2] * 31)          # ragged last round
    assert all(sum(m) == nb for nb, (_, m) in got.items())


# ---- inputs, restatement, bounds ---------------------------------------------------------------------------------------------------------------
def _cases(row, idx):
    """-> [(g32, theta, m, v, plan or None)] of a row's first launch, one entry per tensor (the inputs the GPU module uploads: same seeds)"""
    inp = D.inputs(row, 9000 + idx)
    if row['entry'] in ('pack', 'pack_adam'):
        offs, _ = D.layout(row['tensors'])
        lo, hi, _ = D.segments(row)[0] if row['entry'] == 'pack_adam' else (0, len(row['tensors']), True)
        plans = D.tensor_plans(row, lo, hi)
        out = []
        for k in range(lo, hi):
            t, sl = row['tensors'][k], slice(offs[k], offs[k] + row['tensors'][k]['size'])
            out.append((D.flat_sum(inp['src'][k], inp['src2'][k], t['size']), inp['theta'][sl], inp['m'][sl], inp['v'][sl], (t, plans[k - lo], inp, k)))
        return out
    return [(inp['g'], inp['theta'], inp['m'], inp['v'], None)]


def test_inputs_are_what_the_bounds_need():
    for idx, r in enumerate(ROWS):
        if _elements(r) > SMALL:
            continue
        inp = D.inputs(r, 9000 + idx)
        arrays = [a for a in inp.values() if isinstance(a, np.ndarray)] + [s for key in ('src', 'src2') for s in inp.get(key, []) if s is not None]
        for a in arrays:
            assert a.dtype == np.float32 and np.all(np.isfinite(a)), row_id(r)
            nz = np.abs(a[a != 0])
            assert nz.size == 0 or nz.min() >= 1e-15, (row_id(r), nz.min())                         # no denormal anywhere near
        if r['entry'] == 'rmsprop_step':
            assert np.all(inp['m'] >= 0) and (r['n'] < 16 or np.any((inp['m'] == 0) & (inp['g'] == 0))), row_id(r)
            continue
        for g32, th, m, v, _ in _cases(r, idx):
            assert np.all(v >= 0) and set(np.unique(np.abs(th))) <= {np.float32(x) for x in (0, 1e-3, 1)}, row_id(r)
            assert D.is_warm(r) or (not m.any() and not v.any()), row_id(r)
    # over the table: every gradient scale, exact zeros, zero weights, first steps and warm ones
    g = np.concatenate([c[0] for idx, r in enumerate(ROWS) if r['entry'] == 'pack_adam' and _elements(r) <= SMALL for c in _cases(r, idx)])
    for lo, hi in ((0.5e-6, 1.5e-6 * 10), (0.5e-3, 1.5e-3 * 10), (0.5, 15)):
        assert np.any((np.abs(g) >= lo) & (np.abs(g) < hi))
    assert np.any(g == 0)


def test_restatement_agrees_with_the_oracle():
    from oracle import ops as O
    rng = np.random.default_rng(0)
    g, th, m, v = (rng.standard_normal(257).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    for hp in (D.HP, D.HP99):
        for t in (1, 2, 10, 1000, 100000):
            for gs in (1.0, 0.5, 1.0 / 3):
                lr, b1, b2, eps = (D.f64(h) for h in hp)
                want = O.adam_update(th.astype(np.float64), g.astype(np.float64) * D.f64(gs), m.astype(np.float64), v.astype(np.float64), t, lr, b1, b2, eps)
                got = D.adam64(g, th, m, v, t, hp, gs)
                for a, b in zip((got[2], got[0], got[1]), want):
                    assert np.allclose(a, b, rtol=1e-14, atol=0), (hp, t, gs)
    # SURVEY.md A.5's closed form of a first step: dtheta = -lr g / (|g| + eps / sqrt(1 - beta2))
    lr, b1, b2, eps = (D.f64(h) for h in D.HP)
    _, _, th1 = D.adam64(g, th, 0 * m, 0 * v, 1, D.HP, 1.0)
    g64 = g.astype(np.float64)
    assert np.allclose(th1 - th, -lr * g64 / (np.abs(g64) + eps / np.sqrt(1 - b2)), rtol=1e-10, atol=0)          # (the difference of two weights of size 1)


def test_a_float32_restatement_of_the_kernels_passes_every_bound():
    """the bounds are not so tight that the arithmetic as written misses them: adam1 and rmsprop_k in float32 numpy, without contraction
    and with numpy's own float32 power, stay inside on every row's inputs"""
    worst = {}
    for idx, r in enumerate(ROWS):
        if _elements(r) > SMALL or r['entry'] == 'pack':
            continue
        if r['entry'] == 'rmsprop_step':
            inp = D.inputs(r, 9000 + idx)
            th1, ms1 = D.f32_rms_kernel(inp['g'], inp['theta'], inp['m'], r['hyper'], r['gscale'], r['clip'])
            fr, not_edge, near, moved = D.rms_fractions(inp['g'], inp['theta'], inp['m'], th1, ms1, r['hyper'], r['gscale'], r['clip'])
            assert not_edge == 0 and moved == 0, row_id(r)
            share = D.rms_near_share(inp['g'], inp['theta'], inp['m'], r['hyper'], r['gscale'], r['clip'])
            assert share <= 0.01 and near <= 0.01, (row_id(r), share, near)      # (share: from the float64 reference alone)
        else:
            fr = {}
            for g32, th, m, v, _ in _cases(r, idx):
                th1, m1, v1 = D.f32_kernel(g32, th, m, v, D.ordinal(r), r['hyper'], r['gscale'])
                for k, f in D.adam_fractions(g32, th, m, v, th1, m1, v1, D.ordinal(r), r['hyper'], r['gscale']).items():
                    fr[k] = max(fr.get(k, 0.0), f)
        assert D.within(fr), (row_id(r), fr)
        for k, f in fr.items():
            worst[(r['entry'] == 'rmsprop_step', k)] = max(worst.get((r['entry'] == 'rmsprop_step', k), 0.0), f)
    print('float32 restatement, worst fraction of the bound:', worst)
    assert all(0.05 < f for k, f in worst.items() if k[1] != 'theta_at_0'), worst           # ... nor so loose that they resolve nothing


def _mutant_caught(name, min_ordinal=0):
    """-> the first (row id, output, fraction) at which a kernel implementing the mutant misses a bound by more than a factor of 2"""
    for idx, r in enumerate(ROWS):
        if _elements(r) > SMALL:
            continue
        if name in D.RMS_MUTANTS:
            if r['entry'] != 'rmsprop_step':
                continue
            inp = D.inputs(r, 9000 + idx)
            ms1, th1 = D.rms64(inp['g'], inp['theta'], inp['m'], r['hyper'], r['gscale'], r['clip'], mutant=name)
            fr, not_edge, _, _ = D.rms_fractions(inp['g'], inp['theta'], inp['m'], th1.astype(np.float32), ms1.astype(np.float32), r['hyper'],
                                                 r['gscale'], r['clip'])
            f = max(fr.values())
            if f > 3.0 or not_edge:           # (the float32 rounding of the mutant's own output adds at most one bound)
                return row_id(r), 'theta', f
            continue
        if r['entry'] not in D.ADAM_KEYS or D.ordinal(r) < min_ordinal:
            continue
        t_ord = D.ordinal(r)
        for g32, th, m, v, extra in _cases(r, idx):
            if name in D.ADAM_MUTANTS:
                with np.errstate(invalid='ignore'):
                    m1, v1, th1 = D.adam64(g32, th, m, v, t_ord, r['hyper'], r['gscale'], mutant=name)
            else:
                if extra is None:
                    continue
                t, plan, inp, k = extra
                n = t['size']
                g_mut = g32
                if name == 'slabs_in_reverse_order':
                    rev = lambda s: s[::-1] if s is not None else None
                    g_mut = D.flat_sum(rev(inp['src2'][k]), rev(inp['src'][k]), n) if inp['src2'][k] is not None else D.flat_sum(rev(inp['src'][k]), None, n)
                if name == 'src2_dropped':
                    g_mut = D.flat_sum(inp['src'][k], None, n)
                if name in ('slabs_in_reverse_order', 'src2_dropped'):
                    if not np.array_equal(g_mut.view(np.uint32), g32.view(np.uint32)):           # (flat is held bitwise)
                        return row_id(r), 'flat', np.inf
                    continue
                m1, v1, th1 = D.adam64(g32, th, m, v, t_ord, r['hyper'], r['gscale'])
                keep = np.zeros(n, bool)
                if name == 'tail_untouched' and plan['tail'] is not None:
                    keep[n // 4 * 4:] = True
                if name == 'one_float4_group_untouched' and plan['path'] == 'float4' and plan['chunk'] == D.PACK_CHUNK:
                    keep[3 * 4 * D.K_BLOCK:4 * 4 * D.K_BLOCK] = True                             # (the last of the four groups of the first chunk)
                m1, v1, th1 = np.where(keep, m, m1), np.where(keep, v, v1), np.where(keep, th, th1)
            fr = D.adam_fractions(g32, th, m, v, th1.astype(np.float32), m1.astype(np.float32), v1.astype(np.float32), t_ord, r['hyper'], r['gscale'])
            # (rounding the mutant's float64 outputs to float32 costs at most one of each bound: more than 2 + 1 is more than twice the bound)
            for key, f in fr.items():
                if f > 3.0:
                    return row_id(r), key, f
    return None


def test_the_inputs_tell_sixteen_wrong_kernels_from_the_right_one():
    assert len(D.MUTANTS) == 16
    for name in D.MUTANTS:
        caught = _mutant_caught(name)
        print('%-30s %s' % (name, caught))
        assert caught is not None, 'a kernel with "%s" would pass every row' % name
    late = _mutant_caught('ordinal_minus_1', min_ordinal=2)          # ... and not only through the infinite lr_t of ordinal 0
    print('%-30s %s' % ('ordinal_minus_1, t >= 2', late))
    assert late is not None and np.isfinite(late[2])


def test_no_mutant_means_no_miss():
    assert _mutant_caught(None) is None


def test_a_nan_an_infinity_or_a_negative_moment_in_any_output_fails():
    """one bad element in one output of an otherwise right kernel: the figure of that output is infinite, never NaN, and within() fails"""
    rows = {r['entry']: (idx, r) for idx, r in enumerate(ROWS) if r['n'] == 1025 and (r['entry'] != 'rmsprop_step' or r['clip'])}
    bads = (np.float32('nan'), np.float32('inf'), np.float32('-inf'))
    for e in ('adam_step', 'adam_step_counted'):
        idx, r = rows[e]
        inp = D.inputs(r, 9000 + idx)
        t = D.ordinal(r)
        good = D.f32_kernel(inp['g'], inp['theta'], inp['m'], inp['v'], t, r['hyper'], r['gscale'])
        args = (inp['g'], inp['theta'], inp['m'], inp['v'])
        assert D.within(D.adam_fractions(*args, *good, t, r['hyper'], r['gscale']))
        for which, key in ((0, 'theta'), (1, 'm'), (2, 'v')):
            for bad in bads + ((np.float32(-1e-3),) if key == 'v' else ()):
                for where in (0, 517, 1024, None):                     # one element, or the whole output
                    out = [a.copy() for a in good]
                    out[which][slice(None) if where is None else where] = bad
                    fr = D.adam_fractions(*args, *out, t, r['hyper'], r['gscale'])
                    assert fr[key] == np.inf and not D.within(fr) and not any(np.isnan(f) for f in fr.values()), (e, key, bad, where, fr)
    idx, r = rows['rmsprop_step']
    inp = D.inputs(r, 9000 + idx)
    good = D.f32_rms_kernel(inp['g'], inp['theta'], inp['m'], r['hyper'], r['gscale'], r['clip'])
    args = (inp['g'], inp['theta'], inp['m'])
    assert D.within(D.rms_fractions(*args, *good, r['hyper'], r['gscale'], r['clip'])[0])
    for which, key in ((0, 'theta'), (1, 'ms')):
        for bad in bads + ((np.float32(-1e-3), np.float32(-1e-12)) if key == 'ms' else ()):
            for where in (0, 517, 1024, None):
                out = [a.copy() for a in good]
                out[which][slice(None) if where is None else where] = bad
                fr = D.rms_fractions(*args, *out, r['hyper'], r['gscale'], r['clip'])[0]
                assert fr[key] == np.inf and not D.within(fr) and not any(np.isnan(f) for f in fr.values()), (key, bad, where, fr)
    assert not D.within({'m': 0.5, 'theta': float('nan')}) and not D.within({'theta': float('nan'), 'm': 0.5})


# ---- argument errors, before any launch ------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)
    one = lambda ct, v: (ct * 1)(v)

    def table(parts=1):
        return dict(srcs=one(C.c_void_p, 1 << 20), sizes=one(C.c_size_t, 64), offs=one(C.c_size_t, 0), parts=one(C.c_int, parts), strides=one(C.c_size_t, 0),
                    count=1, flat=p(1 << 21))

    def pack_adam(**kw):
        a = dict(table(kw.pop('parts', 1)), theta=p(1 << 22), m=p(1 << 23), v=p(1 << 24), step=p(1 << 25), arrive=p(1 << 26))
        a.update(kw)
        rc = L.ggan_pack_adam(a['srcs'], a['sizes'], a['offs'], a['parts'], a['strides'], None, None, None, a['count'], a['flat'], a['theta'], a['m'],
                              a['v'], a['step'], a['arrive'], 2e-4, 0.5, 0.999, 1e-8, 1.0, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(srcs=None), 'null'), (dict(sizes=None), 'null'), (dict(offs=None), 'null'), (dict(flat=None), 'null'),
                     (dict(theta=None), 'null'), (dict(m=None), 'null'), (dict(v=None), 'null'), (dict(step=None), 'null'),
                     (dict(count=0), 'count'), (dict(count=D.PACK_MAX + 1), 'count'), (dict(count=-1), 'count'), (dict(parts=0), 'parts'),
                     (dict(flat=p((1 << 21) + 4)), 'buffers must be 16-byte aligned'), (dict(theta=p((1 << 22) + 4)), 'buffers must be 16-byte aligned'),
                     (dict(m=p((1 << 23) + 8)), 'buffers must be 16-byte aligned'), (dict(v=p((1 << 24) + 12)), 'buffers must be 16-byte aligned')):
        rc, msg = pack_adam(**kw)
        assert rc == -1 and 'ggan_pack_adam' in msg and word in msg, (kw, rc, msg)

    def pack(**kw):
        a = dict(table(kw.pop('parts', 1)), bump=None)
        a.update(kw)
        rc = L.ggan_pack_parts2(a['srcs'], a['sizes'], a['offs'], a['parts'], a['strides'], None, None, None, a['count'], a['flat'], a['bump'], None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(srcs=None), 'null'), (dict(sizes=None), 'null'), (dict(offs=None), 'null'), (dict(flat=None), 'null'),
                     (dict(count=0), 'count'), (dict(count=D.PACK_MAX + 1), 'count'), (dict(parts=0), 'parts')):
        rc, msg = pack(**kw)
        assert rc == -1 and 'ggan_pack_parts2' in msg and word in msg, (kw, rc, msg)

    def adam(fn, **kw):
        a = dict(theta=p(1 << 20), g=p(1 << 21), m=p(1 << 22), v=p(1 << 23), n=64, step=p(1 << 24))
        a.update(kw)
        rc = getattr(L, fn)(a['theta'], a['g'], a['m'], a['v'], a['n'], a['step'], 2e-4, 0.5, 0.999, 1e-8, 1.0, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for fn in ('ggan_adam_step', 'ggan_adam_step_counted'):
        for kw, word in [(dict([(k, None)]), 'null') for k in ('theta', 'g', 'm', 'v', 'step')] + \
                        [(dict([(k, p((1 << 20) + 4))]), 'buffers must be 16-byte aligned') for k in ('theta', 'g', 'm', 'v')]:
            rc, msg = adam(fn, **kw)
            assert rc == -1 and fn + ':' in msg and word in msg, (fn, kw, rc, msg)
        assert adam(fn, n=0)[0] == 0                                          # nothing to do is no error (and no launch)

    def rms(**kw):
        a = dict(theta=p(1 << 20), g=p(1 << 21), ms=p(1 << 22), n=64, lo=-0.01, hi=0.01)
        a.update(kw)
        rc = L.ggan_rmsprop_step(a['theta'], a['g'], a['ms'], a['n'], 5e-5, 0.9, 1e-10, 1.0, a['lo'], a['hi'], None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(theta=None), 'null'), (dict(g=None), 'null'), (dict(ms=None), 'null'), (dict(lo=0.02), 'clip')):
        rc, msg = rms(**kw)
        assert rc == -1 and 'ggan_rmsprop_step' in msg and word in msg, (kw, rc, msg)
    assert rms(n=0)[0] == 0
    rc = L.ggan_adam_advance(None, None)
    assert rc == -1 and 'null' in (L.ggan_last_error() or b'').decode()
