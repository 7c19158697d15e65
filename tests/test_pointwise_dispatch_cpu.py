"""The coverage table tests/_pointwise_dispatch.py against csrc/pointwise.hip, without a GPU: every GGAN_LAUNCH label of the unit has a
row and the rows name no other; the constants planned() copies are the source's; written-out launches of the boundary rows equal
planned(); the table reaches every edge it was built for; the float32 restatement of the kernels (run32) passes every bound on every
row while each wrong kernel of MUTANTS misses one by more than a factor of two (or breaks a bitwise stage) on the row MUTANT_ROW names;
FastDiv is exact for every element index of the 32-bit row_lerp rows; and the argument checks answer before any launch."""
import os
import re

import numpy as np

import _pointwise_dispatch as D
from _pointwise_dispatch import ROWS, row_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'graphical_gan_amd', 'csrc')
_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*,\s*[^,]+,\s*[^,]+,\s*\(?(\w+)')


def _read(*names):
    return ''.join(open(os.path.join(CSRC, n)).read() for n in names)


def sites(text):
    """-> [(label, kernel)] of the GGAN_LAUNCH sites of a source text"""
    out = [(m.group(1), m.group(2)) for m in _LAUNCH.finditer(text)]
    assert len(out) == text.count('GGAN_LAUNCH('), 'a launch site the parser cannot read'
    return out


def uncovered(text, rows=ROWS):
    labels = {s[0] for s in sites(text)}
    named = {l[0] for r in rows for l in r['launches'] if not l[0].startswith('gemm_kernel')}
    return sorted(labels - named), sorted(named - labels)


def _inputs(idx):
    return D.inputs(ROWS[idx], 7000 + idx)


# ---- launch sites against rows -------------------------------------------------------------------------------------------------------------
def test_every_site_has_a_row_and_every_row_a_site():
    text = _read('pointwise.hip')
    s = sites(text)
    assert len(s) == 19 and len({k for _, k in s}) == 16           # 16 kernels at 19 sites
    assert uncovered(text) == ([], [])
    by_label = {}
    for label, kernel in s:
        by_label.setdefault(label, []).append(kernel)
    # the two pairs a profiler record could not tell apart have labels of their own, with the old label as a prefix
    assert by_label['row_lerp<32>'] == ['row_lerp32_k'] and by_label['row_lerp<64>'] == ['row_lerp_k']
    assert by_label['chansum<one>'] == ['chansum_part_k'] and by_label['chansum<part>'] == ['chansum_part_k']
    assert by_label['chansum_final'] == ['chansum_final_k', 'chansum_final_k']          # shared: the row's launch list says who issued it
    assert all('row_lerp' in l for l in ('row_lerp<32>', 'row_lerp<64>')) and all('chansum' in l for l in ('chansum<one>', 'chansum<part>'))
    firsts = {l[0] for r in ROWS for l in r['launches'][:1]}
    assert {'colsum_tall', 'chansum<part>'} <= firsts                                   # chansum_final behind each of its two callers
    assert any([l[0] for l in r['launches']] == ['colsum_tall', 'chansum_final'] for r in ROWS)
    assert any([l[0] for l in r['launches']] == ['chansum<part>', 'chansum_final'] for r in ROWS)


def test_a_scratch_copy_with_a_new_or_a_lost_site_is_caught():
    text = _read('pointwise.hip')
    site = 'GGAN_LAUNCH("bias_add"'
    assert text.count(site) == 1
    assert uncovered(text.replace(site, 'GGAN_LAUNCH("bias_add_nhwc"')) == (['bias_add_nhwc'], ['bias_add'])
    assert uncovered(text, [r for r in ROWS if r['entry'] != 'reparam_bwd']) == (['reparam_bwd'], [])


# ---- constants and the plan ------------------------------------------------------------------------------------------------------------------
def test_transcribed_constants_are_the_sources():
    text = _read('pointwise.hip', 'pointwise.h', 'conv.h', 'common.h')
    assert 'constexpr int kBlock = %d;' % D.K_BLOCK in text
    assert 'inline int grid_for(size_t n, int per_thread = %d)' % D.PER_THREAD in text
    assert 'if (b > %d) b = %d;' % (D.GRID_CAP, D.GRID_CAP) in text and 'if (b < 1) b = 1;' in text
    assert text.count('dim3(grid_for(n, %d)), dim3(kBlock)' % D.ACT_PER_THREAD) == 2
    assert text.count('dim3(grid_for(n)), dim3(kBlock)') == 7 and 'dim3(grid_for(total)), dim3(kBlock)' in text
    assert 'int S = (%d + C - 1) / C;' % D.ABC_SPREAD in text and 'if (S > %d) S = %d;' % (D.ABC_MAX_S, D.ABC_MAX_S) in text
    assert 'if (S > N) S = N;' in text and 'if (S > parts_cap / C) S = parts_cap / C;' in text and 'if (S < 1) S = 1;' in text
    assert 'const int ipb = (N + S - 1) / S;' in text and 'S = (N + ipb - 1) / ipb;' in text
    assert 'act_bwd_chansum_k, dim3(C, S), dim3(%d)' % D.ABC_THREADS in text and text.count('j += %d)' % D.ABC_THREADS) == 2
    assert 'const int tiles = cdiv(cols, 64);' in text and 'int P = cdiv(%d, tiles);' % D.TALL_WGS in text
    assert 'if (P > rows / %d) P = rows / %d;' % (D.SLAB_ROWS, D.SLAB_ROWS) in text
    assert 'if (P < 2 || !ws || (size_t)cols * P * sizeof(float) > ws_bytes) return ggan_colsum(x, out, rows, cols, stream);' in text
    assert 'int P = %d / C;' % D.CHAN_WGS in text and 'if (P > N) P = N;' in text
    assert 'if (!ws || (size_t)C * P * sizeof(float) > ws_bytes) P = 1;' in text
    assert 'const int threads = (size_t)N * HW >= %d ? 1024 : 256;' % D.ONE_BIG in text
    assert 'const int threads = HW >= %d ? 256 : (HW >= %d ? 128 : 64);' % (D.HW_256, D.HW_128) in text
    assert 'if ((double)n * cols < 4.0e9) {' in text and D.LERP_LIMIT == 4.0e9
    assert 'f.mul = (d <= 1) ? 0u : (uint32_t)((0x100000000ull / d) + 1ull);' in text
    assert 'return f.d <= 1 ? n : __umulhi(n, f.mul);' in text
    assert 'if (!ws || bytes <= kWsReserved) { bytes = 0; return nullptr; }' in text
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert '#define GGAN_WS_RESERVED %d' % D.WS_RESERVED in hdr
    assert 'GGAN_ACT_NONE = 0, GGAN_ACT_LRELU = 1, GGAN_ACT_RELU = 2, GGAN_ACT_TANH = 3, GGAN_ACT_SIGMOID = 4' in hdr
    assert (D.ACT_NONE, D.ACT_LRELU, D.ACT_RELU, D.ACT_TANH, D.ACT_SIGMOID) == (0, 1, 2, 3, 4)
    gemm = _read('gemm.hip')
    assert 'constexpr int BM = 64, BN = 64, BK = 16' in gemm and 'const int max_sk = K / BK;' in gemm          # the stage rows: K < 32, never split
    build = open(os.path.join(ROOT, 'graphical_gan_amd', 'build.py')).read()
    assert "'-ffp-contract=on'" in build and 'fast-math' not in build                        # what the rounding counts assume


WRITTEN_OUT = {          # (entry, parameters that pick the row) -> its launches, written out by hand
    ('act_fwd', (('n', 1),)): (('act_fwd', 1, (1,), (256,)),),
    ('act_fwd', (('n', 4099),)): (('act_fwd', 1, (2,), (256,)),),
    ('act_fwd', (('n', 2048 * 4096 + 4099),)): (('act_fwd', 1, (2048,), (256,)),),
    ('act_bwd', (('n', 2048 * 4096 + 4099),)): (('act_bwd', 1, (2048,), (256,)),),
    ('act_bwd_chansum', (('N', 9),)): (('act_bwd_chansum', 1, (100, 5), (256,)), ('act_bwd', 1, (226,), (256,))),
    ('act_bwd_chansum', (('N', 200),)): (('act_bwd_chansum', 1, (1, 50), (256,)), ('act_bwd', 1, (13,), (256,))),
    ('act_bwd_chansum', (('N', 40),)): (('act_bwd_chansum', 1, (8, 3), (256,)), ('act_bwd', 1, (1,), (256,))),
    ('bias_add', (('HW', 2048 * 1024 + 1027),)): (('bias_add', 1, (2048,), (256,)),),
    ('axpby', (('n', 1027), ('y', False))): (('axpby', 1, (2,), (256,)),),
    ('row_lerp', (('cols', 63245),)): (('row_lerp<32>', 1, (62,), (256,)),),
    ('row_lerp', (('cols', 63246),)): (('row_lerp<64>', 1, (62,), (256,)),),
    ('row_lerp', (('cols', 1000),)): (('row_lerp<32>', 1, (2048,), (256,)),),
    ('row_lerp', (('cols', 50000),)): (('row_lerp<64>', 1, (98,), (256,)),),
    ('colsum', (('rows', 257), ('cols', 130))): (('colsum', 1, (3,), (64,)),),
    ('colsum_tall', (('rows', 127),)): (('colsum', 1, (2,), (64,)),),
    ('colsum_tall', (('rows', 128), ('cols', 65), ('ws', 'null'))): (('colsum', 1, (2,), (64,)),),
    ('colsum_tall', (('rows', 128), ('cols', 65), ('ws', 'short'))): (('colsum', 1, (2,), (64,)),),
    ('colsum_tall', (('rows', 128), ('cols', 65), ('ws', 'reserved'))): (('colsum', 1, (2,), (64,)),),
    ('colsum_tall', (('rows', 128), ('cols', 65), ('ws', 'full'))): (('colsum_tall', 1, (2, 2), (256,)), ('chansum_final', 1, (17,), (256,))),
    ('colsum_tall', (('rows', 6401),)): (('colsum_tall', 1, (3, 100), (256,)), ('chansum_final', 1, (33,), (256,))),
    ('colsum_tall', (('rows', 65600),)): (('colsum_tall', 1, (1, 1024), (256,)), ('chansum_final', 1, (1,), (256,))),
    ('chansum', (('N', 1), ('C', 3), ('HW', 16383))): (('chansum<one>', 1, (3, 1), (256,)),),
    ('chansum', (('N', 1), ('C', 3), ('HW', 16384))): (('chansum<one>', 1, (3, 1), (1024,)),),
    ('chansum', (('C', 1100), ('HW', 16383))): (('chansum<one>', 1, (1100, 1), (256,)),),
    ('chansum', (('C', 1100), ('HW', 16384))): (('chansum<one>', 1, (1100, 1), (1024,)),),
    ('chansum', (('HW', 5461), ('ws', 'null'))): (('chansum<one>', 1, (2, 1), (256,)),),
    ('chansum', (('HW', 4096), ('ws', 'short'))): (('chansum<one>', 1, (2, 1), (1024,)),),
    ('chansum', (('N', 5), ('HW', 1))): (('chansum<part>', 1, (6, 5), (64,)), ('chansum_final', 1, (2,), (256,))),
    ('chansum', (('N', 5), ('HW', 255))): (('chansum<part>', 1, (6, 5), (64,)), ('chansum_final', 1, (2,), (256,))),
    ('chansum', (('N', 5), ('HW', 256))): (('chansum<part>', 1, (6, 5), (128,)), ('chansum_final', 1, (2,), (256,))),
    ('chansum', (('N', 5), ('HW', 1023))): (('chansum<part>', 1, (6, 5), (128,)), ('chansum_final', 1, (2,), (256,))),
    ('chansum', (('N', 5), ('HW', 1024))): (('chansum<part>', 1, (6, 5), (256,)), ('chansum_final', 1, (2,), (256,))),
    ('chansum', (('N', 400),)): (('chansum<part>', 1, (3, 341), (64,)), ('chansum_final', 1, (1,), (256,))),
    ('stage', (('join', True), ('M', 257))): (('stage_cols<join>', 1, (2,), (256,)), ('gemm_kernel<true, false>', 1, (1, 5, 1), (256,))),
    ('stage', (('join', False), ('M', 16))): (('gemm_kernel<false, false>', 1, (1, 1, 1), (256,)), ('stage_cols<deal>', 1, (1,), (256,))),
}


def _pick(entry, match):
    hits = [r for r in ROWS if r['entry'] == entry and all(r['p'].get(k) == v for k, v in match)]
    assert len(hits) >= 1, (entry, match)
    return hits


def test_recorded_launches_follow_the_dispatch():
    for r in ROWS:
        assert D.planned(r) == r['launches'], row_id(r)
        assert all(len(l) == 4 and l[1] == 1 for l in r['launches'])
        assert len({(l[0], D.threads(l)) for l in r['launches']}) == len(r['launches']), row_id(r)
    for (entry, match), want in WRITTEN_OUT.items():
        for r in _pick(entry, match):
            assert r['launches'] == want, (row_id(r), r['launches'], want)


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    f4 = {'act_fwd': ('x', 'y'), 'act_bwd': ('gy', 'ref', 'gx'), 'act_bwd_chansum': ('gy', 'ref', 'gx', 'gx2'), 'chansum': ('x',)}
    for r in ROWS:
        names = [b[0] for b in D.buffers(r)]
        assert set(r['off']) <= set(names) | {'noise', 'y', 'gz', 'gsd', 'out'}, row_id(r)          # (optional operands a row may leave out)
        for name in f4.get(r['entry'], ()):                        # what a float4 load or an aligned16 guard touches: multiples of 4 floats
            assert r['off'].get(name, 0) % 4 == 0, row_id(r)
        if r['entry'] in ('bias_add', 'cast_scale', 'cast_ring', 'row_lerp', 'colsum', 'colsum_tall', 'reparam_fwd', 'reparam_bwd'):
            assert all(r['off'].get(n, 0) == 1 for n in names if n != 'ctr'), row_id(r)          # scalar loops only: one float off
    big = sorted((max(b[3] for b in D.buffers(r)), r['entry']) for r in ROWS if max(b[3] for b in D.buffers(r)) > 2.2e6)
    # the two capped-grid activation rows, the C = 1100 channel sums at the thread-count threshold and the (3999, 1000) lerp
    assert [e for _, e in big] == ['row_lerp', 'act_bwd', 'act_fwd', 'chansum', 'chansum'], big


# ---- the enumerated edges ------------------------------------------------------------------------------------------------------------------------
def _rows(entry):
    return [r for r in ROWS if r['entry'] == entry]


def test_table_reaches_the_activation_edges():
    for e in ('act_fwd', 'act_bwd'):
        rows = _rows(e)
        assert {r['p']['n'] for r in rows} == {1, 3, 4, 5, 1023, 1024, 1027, 4099, D.ACT_BIG}, e
        for n in (1, 5, 4099):
            assert {r['p']['act'] for r in rows if r['p']['n'] == n} == {0, 1, 2, 3, 4, 5}, (e, n)          # 0 and an unknown code too
        assert {r['p']['n'] % 4 for r in rows} == {0, 1, 3}
        big = [r for r in rows if r['p']['n'] == D.ACT_BIG][0]
        assert D.ACT_BIG == 2048 * 4096 + 4099 and big['launches'][0][2] == (D.GRID_CAP,)
        assert (D.ACT_BIG // 4) > 3 * D.GRID_CAP * D.K_BLOCK and D.ACT_BIG % 4 == 3                          # several trips, and a tail
    planted = set(D.PLANTED.tolist())
    assert planted == {0.0, 1e-6 * 1.0, -1e-6, 20.0, -20.0, 80.0, -80.0, 100.0, -100.0, 1e4, -1e4} or len(D.PLANTED) == 12
    assert np.signbit(D.PLANTED[1]) and not np.signbit(D.PLANTED[0])
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'act_fwd' and r['p']['n'] >= 1023:
            x = _inputs(idx)['x']
            assert all(np.any(x.view(np.uint32) == v.view(np.uint32)) for v in D.PLANTED), row_id(r)
        if r['entry'] == 'act_bwd' and 1023 <= r['p']['n'] <= 4099:
            ref = _inputs(idx)['ref']
            z = ref == 0
            assert 0.05 < z.mean() < 0.2 and np.any(np.signbit(ref[z])) and np.any(~np.signbit(ref[z])), row_id(r)
    # the tail of the two kernels: at most 3 elements, fewer than the smallest grid's threads -- why 'tail_one_trip' is the same kernel
    assert D.EQUIVALENT_MUTANTS == ('tail_one_trip', 'tail_from_n4') and 3 < D.K_BLOCK and not set(D.EQUIVALENT_MUTANTS) & set(D.MUTANTS)


def test_the_two_tail_mutants_are_the_same_kernel():
    """why EQUIVALENT_MUTANTS cannot be caught: on every length of the table the tail loop `for (j = start + i; j < n; j += stride)`
    reaches each of the last n % 4 elements in its FIRST trip when start = (n4 << 2), and still reaches each of them (after elements
    the float4 loop already stored, with the same values) when start = n4"""
    for n in sorted({r['p']['n'] for r in _rows('act_fwd')}):
        threads = D.grid_for(n, D.ACT_PER_THREAD) * D.K_BLOCK
        n4 = n >> 2
        tail = set(range(4 * n4, n))
        assert len(tail) == n % 4 and tail <= {4 * n4 + i for i in range(threads)}, n                 # 'tail_one_trip'
        # 'tail_from_n4': thread i = (j - n4) % threads reaches j = n4 + i + k threads in trip k = (j - n4) // threads
        assert all(j >= n4 and 0 <= (j - n4) % threads < threads for j in tail), n


def test_table_reaches_every_clamp_of_act_bwd_chansum():
    rows = _rows('act_bwd_chansum')
    plans = [D.abc_plan(r['p']['N'], r['p']['C'], r['p']['cap']) for r in rows]
    assert {pl[1] for pl in plans} == {'spread', 'N', 'cap', '64'}                    # 'one' cannot be reached: see below
    assert any(pl[3] < pl[0] for pl in plans) and (6, 'spread', 2, 5) in plans       # the recomputed S shrinks: N = 9 with a first S of 6
    assert any(r['p']['N'] % pl[2] for r, pl in zip(rows, plans))                     # a short last slab
    assert {r['p']['HW'] for r in rows} >= {4, 1024, 1028, 1, 255, 259} and {r['p']['C'] for r in rows} >= {1, 600}
    assert any(r['p']['cap'] > pl[3] * r['p']['C'] for r, pl in zip(rows, plans))     # slabs that keep their NaN
    assert all(r['p']['cap'] >= r['p']['C'] for r in rows)
    # S < 1 needs cdiv(512, C) < 1, N < 1 or parts_cap / C < 1: the guards N > 0, C > 0, parts_cap >= C exclude all three
    for C in (1, 2, 511, 512, 513, 600, 100000):
        for N in (1, 2, 1000):
            for cap in (C, C + 1, 70 * C):
                assert D.abc_plan(N, C, cap)[1] != 'one'


def test_table_reaches_the_remaining_pointwise_edges():
    assert {(r['p']['N'], r['p']['C'], r['p']['HW']) for r in _rows('bias_add')} >= {(1, 1, 1), (3, 5, 1), (2, 1, 7), (3, 5, 7), (1, 1, D.BIG)}
    assert D.BIG == 2048 * 1024 + 1027
    cs = _rows('cast_scale')
    assert {(r['p']['div'], r['p']['mul']) for r in cs} >= {(255.0, 2.0), (256.0, 1.0)} and {r['p']['noise'] for r in cs} == {True, False}
    assert {r['p']['n'] for r in cs} >= {1, 257, D.BIG}
    vals = set(D.CAST_EDGES.tolist())
    assert set(range(256)) <= vals and {2 ** 24 + 1, D.I32_MIN, D.I32_MAX, -1} <= vals
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'cast_scale' and r['p']['n'] >= 257:
            have = set(_inputs(idx)['x'].tolist())
            assert set(range(256)) <= have and (vals <= have if r['p']['n'] >= 300 else have - set(range(256))), row_id(r)
    ring = _rows('cast_ring')
    assert {r['p']['nslots'] for r in ring} == {1, 3, 7}
    kinds = {(r['p']['ctr_a'] is None, r['p']['ctr_b'] is None) for r in ring}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}
    sums = [(r['p']['ctr_a'] or 0) + (r['p']['ctr_b'] or 0) + r['p']['offset'] for r in ring]
    assert -1 in sums and any(s < 0 and s % r['p']['nslots'] == 0 for s, r in zip(sums, ring)) and any(s > 2 ** 32 for s in sums)
    assert any(r['p']['ctr_a'] == r['p']['ctr_b'] == D.I32_MAX and r['p']['offset'] > 0 for r in ring)
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'cast_ring':
            x = _inputs(idx)['ring'].reshape(r['p']['nslots'], -1)
            assert len({row.tobytes() for row in x}) == r['p']['nslots'], row_id(r)          # every slot holds other data
            assert 0 <= D.ring_slot(r['p']) < r['p']['nslots']
    ax = _rows('axpby')
    assert {r['p']['abc'] for r in ax} >= {(1.0, 1.0, 0.0), (0.5, -2.0, 0.25), (0.0, 0.0, 3.0)} and {r['p']['n'] for r in ax} == {1, 5, 1027, D.BIG}
    assert any(not r['p']['y'] and not r['p']['inplace'] for r in ax) and any(not r['p']['y'] and r['p']['inplace'] and r['p']['n'] == 1 for r in ax)
    lerp = {(r['p']['rows'], r['p']['cols']): r['launches'][0][0] for r in _rows('row_lerp')}
    assert lerp == {(64, 300): 'row_lerp<32>', (5, 1): 'row_lerp<32>', (3, 2): 'row_lerp<32>', (7, 3): 'row_lerp<32>', (3999, 1000): 'row_lerp<32>',
                    (1, 63245): 'row_lerp<32>', (1, 63246): 'row_lerp<64>', (2, 50000): 'row_lerp<64>'}
    assert 63245 ** 2 < 4.0e9 <= 63246 ** 2 and 3999 * 1000 ** 2 < 4.0e9 <= 2 * 50000 ** 2          # the two boundary rows on opposite sides
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'row_lerp':
            a = _inputs(idx)['alpha']
            assert np.any(a == 0) and (r['p']['rows'] == 1 or np.any(a == 1)), row_id(r)
    assert {(r['p']['rows'], r['p']['cols']) for r in _rows('colsum')} == {(a, b) for a in (1, 2, 257) for b in (1, 63, 64, 65, 130)}
    rp = _rows('reparam_bwd')
    assert {(r['p']['gz'], r['p']['gsd']) for r in rp} == {(True, True), (False, True), (True, False)}
    assert {r['p']['n'] for r in rp} == {r['p']['n'] for r in _rows('reparam_fwd')} == {1, 5, 1027, D.BIG}
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'reparam_fwd' and r['p']['n'] >= 1027:
            ls = _inputs(idx)['log_std']
            assert ls.min() == -20 and ls.max() == 80 and np.any((ls == 0) & np.signbit(ls)) and np.any((ls == 0) & ~np.signbit(ls))
    st = _rows('stage')
    for join in (True, False):
        rc = {np.prod(D.stage_shape(r['p'])) for r in st if r['p']['join'] == join}
        assert rc == {255, 256, 257}, (join, rc)
        sp = {(r['p']['split'] == 1, r['p']['split'] == D.stage_shape(r['p'])[1] - 1) for r in st if r['p']['join'] == join}
        assert (True, False) in sp and (False, True) in sp
    assert all(r['p']['split'] % 64 for r in st) and all(r['p']['K'] < 32 and r['p']['M'] * 0 == 0 for r in st)
    assert all(r['p']['Nn'] > 1 for r in st)                                          # (N = 1 would be gemv_rows_k)


def test_table_reaches_the_reduction_edges():
    tall = _rows('colsum_tall')
    falls = [r for r in tall if D.tall_plan(r) is None]
    assert {r['p']['ws'] for r in falls} == {'full', 'null', 'short', 'reserved'}
    assert any(r['p']['rows'] // 64 < 2 and r['p']['ws'] == 'full' for r in falls)
    short = [r for r in falls if r['p']['ws'] == 'short'][0]
    assert D.ws_floats(short) == 65 * 2 - 1
    plans = {(r['p']['rows'], r['p']['cols']): D.tall_plan(r) for r in tall if D.tall_plan(r)}
    assert plans[(6401, 130)] == (100, 65) and plans[(65600, 3)] == (1024, 65) and plans[(128, 65)] == (2, 64) and plans[(128, 64)] == (2, 64)
    assert 98 * 65 < 6401 < 99 * 65                                                   # slab 98 short, slab 99 holds no rows
    assert any(P > 64 for P, _ in plans.values()) and any(rps % 4 for _, rps in plans.values())
    ch = _rows('chansum')
    one = [(r['p'], D.chan_plan(r)) for r in ch if D.chan_plan(r)[0] == 1]
    for cause in (lambda p: p['N'] == 1 and p['C'] == 3, lambda p: p['C'] == 1100, lambda p: p['ws'] == 'null', lambda p: p['ws'] == 'short'):
        assert {p['N'] * p['HW'] for p, _ in one if cause(p)} == {16383, 16384}
        assert {pl[1] for p, pl in one if cause(p)} == {256, 1024}
    two = {r['p']['HW']: D.chan_plan(r)[1] for r in ch if D.chan_plan(r)[0] > 1 and r['p']['N'] == 5 and r['p']['C'] == 6}
    assert two == {1: 64, 255: 64, 256: 128, 1023: 128, 1024: 256}
    assert any(r['p']['C'] % 4 for r in ch if D.chan_plan(r)[0] > 1) and any(r['p']['C'] % 4 == 0 for r in ch if D.chan_plan(r)[0] > 1)
    p341 = [r for r in ch if r['p']['N'] == 400][0]
    assert D.chan_plan(p341) == (341, 64) and D.cdiv(341, 64) == 6
    assert {r['p']['HW'] % 4 == 0 for r in ch if D.chan_plan(r)[0] > 1} == {True, False}


# ---- FastDiv ---------------------------------------------------------------------------------------------------------------------------------
def test_fastdiv_is_exact_for_every_element_index_of_the_32_bit_rows():
    """mul = floor(2^32 / d) + 1 = (2^32 + e) / d with 0 < e <= d, so n mul / 2^32 = n / d + n e / (d 2^32): the floor is that of n / d as
    long as the excess n e / (d 2^32) stays below 1 / d, the distance of n / d's fraction from 1 -- n e < 2^32, which n d < 2^32 gives.
    An element index is below rows cols, so n cols < rows cols^2 < 4e9 < 2^32: exact on every row the predicate sends to the 32-bit
    kernel.  Evaluated here for every index of every such row; one less in the multiplier fails at the first multiple of d."""
    seen = 0
    for r in _rows('row_lerp'):
        rows, cols = r['p']['rows'], r['p']['cols']
        if not D.lerp_is_32(rows, cols):
            continue
        seen += 1
        assert rows * cols * cols < 4.0e9 < 2 ** 32
        mul, d = D.make_fastdiv(cols)
        assert d <= 1 or 0 < mul * d - 2 ** 32 <= d                                   # the multiplier's excess is at most cols
        j = np.arange(rows * cols, dtype=np.uint64)
        assert np.array_equal(D.fdiv(j, (mul, d)), j // np.uint64(cols)), (rows, cols)
        if cols == 300:
            assert not np.array_equal(D.fdiv(j, (mul, d), 'fdiv_multiplier_minus_1'), j // np.uint64(cols))
    assert seen == 6


# ---- the float32 restatement, the bounds, the mutants -----------------------------------------------------------------------------------------
def test_a_float32_restatement_of_the_kernels_passes_every_bound():
    worst = {}
    for idx, r in enumerate(ROWS):
        inp = _inputs(idx)
        fr = D.check(r, inp, D.run32(r, inp))
        assert D.within(fr), (row_id(r), fr)
        for k, f in fr.items():
            worst[(r['entry'], k)] = max(worst.get((r['entry'], k), 0.0), f)
    print('float32 restatement, worst fraction of the bound:', {k: round(v, 3) for k, v in worst.items() if v})
    # ... nor are the counted bounds so loose that they resolve nothing
    for key in (('act_bwd', 'gx'), ('axpby', 'out'), ('row_lerp', 'out'), ('colsum', 'out'), ('reparam_bwd', 'glog'), ('act_bwd_chansum', 'parts')):
        assert worst[key] > 0.02, (key, worst[key])


def test_every_wrong_kernel_is_caught_on_its_row():
    index = {row_id(r): i for i, r in enumerate(ROWS)}
    assert len(D.MUTANTS) >= 21
    for name, rid in D.MUTANT_ROW.items():
        idx = index[rid]
        inp = _inputs(idx)
        right = D.check(ROWS[idx], inp, D.run32(ROWS[idx], inp))
        wrong = D.check(ROWS[idx], inp, D.run32(ROWS[idx], inp, mutant=name))
        print('%-34s %-60s %s' % (name, rid, {k: v for k, v in wrong.items() if v > 1}))
        assert D.within(right) and max(wrong.values()) > 2.0, 'a kernel with "%s" would pass %s' % (name, rid)


def test_a_nan_or_an_infinity_in_any_output_fails():
    for idx, r in enumerate(ROWS):
        if max(b[3] for b in D.buffers(r)) > 5000:
            continue
        inp = _inputs(idx)
        good = D.run32(r, inp)
        for key in good:
            if key in ('n_parts', 'ctr') or np.asarray(good[key]).size == 0:
                continue
            for bad in (np.float32('nan'), np.float32('inf')):
                out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
                out[key][0] = bad
                fr = D.check(r, inp, out)
                assert not D.within(fr) and not any(np.isnan(f) for f in fr.values()), (row_id(r), key, bad, fr)


# ---- argument errors, before any launch ------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    pointer = lambda k: (k + 1) << 20           # (never dereferenced: every case fails its checks first)
    assert len(D.REJECTED) >= 60
    for case in D.REJECTED:
        rc, msg, n_parts = D.call(L, case, pointer)
        assert rc != 0 and case[0] + ':' in msg and case[2] in msg and n_parts == -7, (case, rc, msg)
    for case in D.EMPTY:
        assert D.call(L, case, pointer)[0] == 0, case                                     # nothing to do is no error (and no launch)
    fns = {c[0] for c in D.REJECTED}
    assert fns == set(D.GOOD)
    assert any(c[0] == 'ggan_reparam_bwd' and c[1][0] is None and c[1][1] is None for c in D.REJECTED)
    assert any(c[0] == 'ggan_act_bwd_chansum' and c[1][4] < c[1][7] for c in D.REJECTED)            # parts_cap < C
