"""The coverage table tests/_conv_dispatch.py against the sources: every kernel name the conv2d family launches (the names the
instance lists CORR_EACH of csrc/conv_corr.hip, WGRAD4_EACH of conv_wgrad.hip and DG16_EACH of conv_dg16.hip spell through their
stringising forms, and the literal first arguments of GGAN_LAUNCH in those files, conv_thin.hip and conv_naive.hip) has a row, no
row names a kernel the sources no longer launch, and the table keeps the cases it was written for.  Reads the project's own sources
for kernel names only."""
import os
import re


from _conv_dispatch import ROWS, row_id

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graphical_gan_amd', 'csrc')
FAMILY = ('conv_corr.hip', 'conv_wgrad.hip', 'conv_thin.hip', 'conv_naive.hip')
HELPERS = ('conv_api.hip', 'optim.hip', 'pointwise.hip')          # pad_width_k, pack, chansum: only ever in a row's `also`

_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*(\(\s*MODE == 0 \? "([^"]+)" : "([^"]+)"\s*\)|"([^"]+)")\s*,')


def launched_names(text):
    """the kernel names a source text passes to GGAN_LAUNCH as string literals"""
    out = set()
    for m in _LAUNCH.finditer(text):
        out.update(n for n in (m.group(2), m.group(3), m.group(4)) if n)
    return out


_FORM = re.compile(r'"([^"\n]*)"((?:\s*#\w+\s*"[^"\n]*")+)')
EACH = (('conv_corr.hip', 'CORR_EACH', 'corr_kernel<', 1), ('conv_wgrad.hip', 'WGRAD4_EACH', 'wgrad4_kernel<', 2),
        ('conv_dg16.hip', 'DG16_EACH', 'dg16_kernel<', 2))          # (file, instance list, name prefix, stringising forms)


def each_names(text, each, prefix, nforms):
    """the names an instance list spells: every `X(..)` entry of `#define <each>(X) X(..) X(..)` (continuation lines included) put
    through every stringising form `"<prefix>" #A ", " #B ">"` of the text; #A, #B are parameters of the `#define` the form stands in"""
    body = re.search(r'#define %s\(X\)((?:.*\\\n)*.*)' % each, text).group(1)
    entries = [[a.strip() for a in e.split(',')] for e in re.findall(r'X\(([^()]*)\)', body)]
    forms = [f for f in _FORM.finditer(text) if f.group(1).startswith(prefix)]
    assert entries and len(forms) == nforms, (each, entries, [f.group(0) for f in forms])
    names = set()
    for f in forms:
        params = [p.strip() for p in re.findall(r'#define \w+\(([^)]*)\)', text[:f.start()])[-1].split(',')]
        for e in entries:
            assert len(e) == len(params), (each, e, params)
            value = dict(zip(params, e))
            names.add(f.group(1) + ''.join(value[p] + lit for p, lit in re.findall(r'#(\w+)\s*"([^"\n]*)"', f.group(2))))
    return names


def _read(name, csrc=CSRC):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def family_names(csrc=CSRC):
    names = set()
    for f in FAMILY:
        names |= launched_names(_read(f, csrc))
    for f, each, prefix, nforms in EACH:
        names |= each_names(_read(f, csrc), each, prefix, nforms)
    return names


def uncovered(csrc=CSRC):
    """-> (launched names without a row, row kernels the sources do not launch)"""
    names = family_names(csrc)
    rows = set(r['kernel'] for r in ROWS)
    also = set(a for r in ROWS for a in r['also'])
    return sorted(n for n in names if n not in rows and n not in also), sorted(rows - names)


def test_parser_reads_both_arms_and_plain_literals():
    text = ('case 1: GGAN_LAUNCH((MODE == 0 ? "k<0, 1, false>" : "k<2, 1, false>"), fl, ab, (k<MODE, 1>), grid, dim3(256), shmem, s, P); break;\n'
            'GGAN_LAUNCH("other_k", 0, 0, other_k, dim3(1), dim3(256), 0, s, P);\n'
            '    if (P.MT == 8) { GGAN_LAUNCH("thin", fl, 0, (thin<NT_, true, 8>), grid, dim3(512), shmem, s, P); } \\\n')
    assert launched_names(text) == {'k<0, 1, false>', 'k<2, 1, false>', 'other_k', 'thin'}


def test_list_reader_follows_continuation_lines_and_every_form():
    text = ('#define K_EACH(X)   \\\n    X(0, 2, false) X(1, 4, true) \\\n    X(2, 8, true)\n'
            '#define K_ATTR(A, B, C) opt_in(k<A, B, C>);\n'
            '#define K_INST(MODE, PW, X4) {MODE, PW, X4, "k<" #MODE ", " #PW ", " #X4 ">", k<MODE, PW, X4>},\n'
            '#define W_EACH(X) X(8) X(16)\n'
            '#define W_CASE(GW) if (w == GW) { GGAN_LAUNCH("w4<" #GW ">", fl, ab, w4<GW>, grid, dim3(256), shmem, s, P); } \\\n'
            '    else { GGAN_LAUNCH("w4<" #GW ", true>", fl, ab, (w4<GW, true>), grid, dim3(512), shmem, s, P); }\n')
    assert each_names(text, 'K_EACH', 'k<', 1) == {'k<0, 2, false>', 'k<1, 4, true>', 'k<2, 8, true>'}
    assert each_names(text, 'W_EACH', 'w4<', 2) == {'w4<8>', 'w4<16>', 'w4<8, true>', 'w4<16, true>'}
    assert not launched_names(text)


def test_every_launched_kernel_has_a_row_and_every_row_a_launch():
    names = family_names()
    assert len(names) >= 40, sorted(names)
    rows = set(r['kernel'] for r in ROWS)
    also = set(a for r in ROWS for a in r['also'])
    missing, stale = uncovered()
    assert not missing, 'kernels launched by csrc/conv_*.hip without a row in tests/_conv_dispatch.py: %s' % missing
    assert not stale, 'rows of tests/_conv_dispatch.py name kernels the sources no longer launch: %s' % stale
    helpers = set()
    for f in HELPERS:
        helpers |= launched_names(_read(f))
    unknown = sorted(also - names - helpers)
    assert not unknown, unknown
    # the split-K reductions are only ever helpers
    assert {'splitk_reduce_k', 'splitk_reduce_small_k'} <= also and not ({'splitk_reduce_k', 'splitk_reduce_small_k'} & rows)


def test_a_scratch_copy_with_one_more_instance_is_caught(tmp_path):
    """a copy of the sources with one more corr_kernel launch and one launch fewer: both directions are reported"""
    for f in FAMILY + ('conv_dg16.hip',):
        text = _read(f)
        if f == 'conv_corr.hip':
            text += 'case 3: GGAN_LAUNCH("corr_kernel<1, 1, 1, 4, 4, false>", fl, ab, (corr_kernel<1, 1, 1, 4, 4>), grid, dim3(256), shmem, s, P); break;\n'
        if f == 'conv_naive.hip':
            text = text.replace('GGAN_LAUNCH("conv_wgrad_naive"', 'GGAN_LAUNCH("conv_wgrad_plain"')
        (tmp_path / f).write_text(text)
    missing, stale = uncovered(str(tmp_path))
    assert missing == ['conv_wgrad_plain', 'corr_kernel<1, 1, 1, 4, 4, false>'] and stale == ['conv_wgrad_naive'], (missing, stale)


def test_a_scratch_copy_with_one_more_list_entry_is_caught(tmp_path):
    """a copy of the sources with one more X(..) entry in the corr and the wgrad4 instance lists and one entry fewer in the dg16 list"""
    for f in FAMILY + ('conv_dg16.hip',):
        text = _read(f)
        if f == 'conv_corr.hip':
            assert text.count('X(1, 2, 1, 2, 4, false)') == 1
            text = text.replace('X(1, 2, 1, 2, 4, false)', 'X(1, 2, 1, 2, 4, false) X(1, 1, 1, 4, 4, false)')
        if f == 'conv_wgrad.hip':
            assert text.count('X(32) X(64)') == 1
            text = text.replace('X(32) X(64)', 'X(32) X(64) X(128)')
        if f == 'conv_dg16.hip':
            assert text.count(' X(24, 2)') == 1
            text = text.replace(' X(24, 2)', '')
        (tmp_path / f).write_text(text)
    missing, stale = uncovered(str(tmp_path))
    assert missing == ['corr_kernel<1, 1, 1, 4, 4, false>', 'wgrad4_kernel<128, true>', 'wgrad4_kernel<128>'], missing
    assert stale == ['dg16_kernel<24, 2, false>', 'dg16_kernel<24, 2, true>'], stale


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids)
    ops = {'fwd', 'fwd_masked', 'fwd_cast', 'dgrad', 'dgrad_masked', 'dgrad_bias_act', 'wgrad', 'wgrad_act', 'wgrad_parts'}
    switches = {'GGAN_DG16', 'GGAN_DG16_FORCE', 'GGAN_DG16_KQ', 'GGAN_NO_THIN', 'GGAN_WGRAD_SPLIT', 'GGAN_WGRAD_W4', 'GGAN_FWD_SK', 'GGAN_DGRAD_SK',
                'GGAN_WGRAD_SK'}
    for r in ROWS:
        assert r['op'] in ops and set(r['env']) <= switches, r
        N, Ci, H, W, Co, pad = r['geom']
        assert pad == 'SAME' and N <= 16 and max(H, W) <= 132 and N * Ci * H * W * Co <= 2 ** 24, r       # small: a few seconds at most
        assert r['tiles'] >= 1 and r['sk'] >= 1 and r['block'] in (256, 512, 1024) and r['target'] >= 0, r
        reduces = [a for a in r['also'] if a.startswith('splitk_reduce')]
        if r['op'] == 'wgrad_parts':
            assert 'pack' in r['also'] and not reduces, r
        else:
            assert len(reduces) == (1 if r['sk'] > 1 else 0), r
        if r['kernel'].startswith('corr_kernel<'):
            mode, wm, wn, ks, pw, x4 = r['kernel'][len('corr_kernel<'):-1].split(', ')
            assert r['op'].startswith('fwd') == (mode == '0') and r['plan']['xq'] == (4 if x4 == 'true' else 1), r
            assert r['block'] == 64 * int(wm) * int(wn) * int(ks), r
            if mode != '0':
                assert r['env'].get('GGAN_DG16') == '0' or r['geom'][1] % 16 or r['geom'][4] % 16, r     # else conv_dg16.hip may take it


def _cdiv(a, b):
    return -(-a // b)


def test_recorded_xcd_order_follows_the_planners_formula():
    """plan_and_launch: with (gx * gy) % 8 == 0 the eight L2s fetch 8 * input / p + filter * p for p pixel-tile groups; p is the cheapest
    admissible power of two if it beats the plain order by 10 %"""
    seen = set()
    for r in ROWS:
        if 'plan' not in r:
            continue
        N, Ci, H, W, Co, _ = r['geom']
        mode, wm, wn = (int(v) for v in r['kernel'][len('corr_kernel<'):].split(', ')[:3])
        TI, TR, TC = r['plan']['tile']
        Ho, Wo = _cdiv(H, 2), _cdiv(W, 2)             # forward: the output grid; data gradient: the largest parity class grid
        gx, gy = _cdiv(N, TI) * _cdiv(Ho, TR) * _cdiv(Wo, TC), _cdiv(Co if mode == 0 else Ci, 32 * wn)
        assert gx * gy * (2 if mode == 1 else 1) == r['tiles'], r
        in_bytes = 4.0 * N * (Ci * H * W if mode == 0 else Co * Ho * Wo)
        w_bytes = 100.0 * Ci * Co
        p_best = 0
        if (gx * gy) % 8 == 0:
            best = in_bytes + 8.0 * w_bytes if gx % 8 == 0 else 8.0 * (in_bytes + w_bytes)
            for p in (1, 2, 4, 8):
                if gx % p or gy % (8 // p):
                    continue
                cost = 8.0 * in_bytes / p + w_bytes * p
                if cost < 0.9 * best:
                    best, p_best = cost, p
        assert r['plan']['xcd_p'] == p_best, (r, p_best)
        seen.add((mode, p_best))
        if p_best in (2, 4) and gx // p_best > 1 and gy // (8 // p_best) > 1:
            seen.add((mode, 'slots'))
    for mode in (0, 1, 2):                               # per kind: plain order, and an order that permutes both tile axes
        assert (mode, 0) in seen and ((mode, 2) in seen or (mode, 4) in seen), (mode, sorted(seen, key=str))
        assert (mode, 'slots') in seen, mode             # ... on a grid with several slots per XCD group on both axes


def test_table_keeps_the_cases_it_was_written_for():
    corr = [r for r in ROWS if r['kernel'].startswith('corr_kernel<')]
    chunk = lambda r: 2 * int(r['kernel'].split(', ')[3]) * int(r['kernel'].split(', ')[4])        # reduction channels per chunk: 2 * KS * PW
    for mode in '012':
        rows = [r for r in corr if r['kernel'].startswith('corr_kernel<' + mode)]
        red = lambda r: r['geom'][1] if mode == '0' else r['geom'][4]
        out = lambda r: r['geom'][4] if mode == '0' else r['geom'][1]
        assert any(red(r) % chunk(r) for r in rows), mode                                         # reduction-channel tail
        assert any(out(r) % (32 * int(r['kernel'].split(', ')[2])) for r in rows), mode           # output channels not a multiple of the tile
        assert any('splitk_reduce_small_k' in r['also'] for r in rows) and any('splitk_reduce_k' in r['also'] for r in rows), mode
        assert any(r['sk'] == 1 for r in rows), mode
        assert any(red(r) < 8 for r in rows), mode                                                 # small-channel override
    fwd_small = [r for r in corr if r['op'] == 'fwd' and 5 <= r['geom'][1] <= 7]
    assert any(r['geom'][4] <= 32 for r in fwd_small) and any(r['geom'][4] > 32 for r in fwd_small)
    assert any(r['op'] == 'fwd_masked' for r in corr) and any(r['op'] == 'dgrad_masked' for r in corr) and any(r['op'] == 'dgrad_bias_act' for r in corr)
    widened = [r for r in ROWS if 'pad_width_k' in r['also']]
    assert {r['geom'][3] for r in widened} >= {28, 14, 7} and all(r['kernel'].startswith('wgrad') for r in widened)
    thin_ops = {(r['kernel'], r['op']) for r in ROWS if r['kernel'].startswith('thin_')}
    assert {('thin_fwd_kernel', 'fwd'), ('thin_fwd_kernel', 'fwd_cast'), ('thin_fwd_kernel', 'fwd_masked'), ('thin_dgrad_kernel', 'dgrad'),
            ('thin_dgrad_kernel', 'dgrad_masked'), ('thin_wgrad_kernel', 'wgrad'), ('thin_wgrad_kernel', 'wgrad_parts')} <= thin_ops
    for n in ('conv_fwd_naive', 'conv_dgrad_naive', 'conv_wgrad_naive'):
        assert any(r['kernel'] == n and not r['also'] for r in ROWS), n
    wg = {(r['kernel'], r['op']) for r in ROWS if r['kernel'].startswith('wgrad')}
    assert {o for _, o in wg} == {'wgrad', 'wgrad_act', 'wgrad_parts'}
