"""The coverage table tests/_gemm_dispatch.py against csrc/gemm.hip: every (kernel name, variant) pair the launch macros can produce --
the GGAN_GEMM_CASE and GGAN_SKINNY_NS uses with their literal name arguments and the FAST / NS arms of the macro bodies, and the
literal GGAN_LAUNCH names -- has a row, and no row names a pair the source no longer produces; every row's recorded plan follows from a
Python transcription of gemm_plan's split choice and of gemm_launch's skinny predicate; the table keeps the cases it was written for;
the exact data of the generic-loader rows is exact.  Reads the project's own source for names only."""
import os
import re

import numpy as np

import _gemm_dispatch as D
from _gemm_dispatch import ROWS, BIG_ROWS, row_id, FF, FT, TF, TT, FT1, TF2

GEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graphical_gan_amd', 'csrc', 'gemm.hip')
HEADS = ('critic_head_fwd', 'critic_head_fwd_bce', 'critic_head_bwd', 'critic_head_bwd_tail')
ENTRIES = ('gemm', 'gemm_split', 'gemm_colsum', 'linear_bwd_data_act', 'linear_bwd_weight_act') + HEADS
REDUCES = {'splitk_reduce_k', 'splitk_reduce_small_k'}


def _read(path=GEMM_HIP):
    with open(path) as f:
        return f.read()


# ---- names against rows --------------------------------------------------------------------------------------------------------------
_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*(NAME_)?\s*,\s*[^,]+,\s*[^,]+,\s*\(?\s*(\w+)(?:<([^()]*)>)?\)?\s*,')


def macro_pairs(text, macro, value_of):
    """-> {(name, variant)}: every GGAN_LAUNCH("<prefix>" NAME_, ..., (kernel<.., V>), ...) arm of `#define <macro>(..)` crossed with the
    literal name argument of every use of the macro; the variant V is the kernel's last template argument"""
    body = re.search(r'#define %s\(([^)]*)\)((?:.*\\\n)*.*)' % macro, text)
    arms = [(m.group(1), m.group(4).split(',')[-1].strip()) for m in _LAUNCH.finditer(body.group(2)) if m.group(2)]
    uses = re.findall(r'%s\([^"\n]*"([^"]+)"\s*\)' % macro, text[body.end():])
    assert arms and uses, (macro, arms, uses)
    return {(prefix + name, value_of(v)) for prefix, v in arms for name in uses}


def source_pairs(text):
    """every (name, variant) the file can launch; variant None for the plain literal names"""
    pairs = macro_pairs(text, 'GGAN_GEMM_CASE', int) | macro_pairs(text, 'GGAN_SKINNY_NS', int)
    defs = [m.span() for m in re.finditer(r'#define GGAN_(?:GEMM_CASE|SKINNY_NS)\((?:.*\\\n)*.*', text)]
    for m in _LAUNCH.finditer(text):
        if not m.group(2) and not any(a <= m.start() < b for a, b in defs):
            pairs.add((m.group(1), None))
    return pairs


def row_pairs(rows):
    out = set()
    for r in rows:
        x = r['expect'][0]
        if r['kernel'].startswith('gemm_kernel'):
            out.add((r['kernel'], x['fast']))
        elif r['kernel'].startswith('gemm_skinny_k'):
            out.add((r['kernel'], x['ns']))
        else:
            out.add((r['kernel'], None))
    return out


def uncovered(text):
    """-> (pairs the source launches without a row, pairs rows name that the source does not launch)"""
    src = source_pairs(text)
    rows = row_pairs(ROWS + BIG_ROWS)
    also = {(a, None) for r in ROWS + BIG_ROWS for a in r['also']}
    key = lambda p: (p[0], -1 if p[1] is None else p[1])
    return sorted((p for p in src if p not in rows and p not in also), key=key), sorted(rows - src, key=key)


def test_parser_reads_macro_arms_uses_and_plain_literals():
    text = ('#define GGAN_GEMM_CASE(TA_, NAME_)   \\\n    do {   \\\n'
            '        if (w8) { GGAN_LAUNCH("k8" NAME_, fl, 0, (k8<TA_, 1>), grid, dim3(512), 0, s, P); }   \\\n'
            '        else { GGAN_LAUNCH("k" NAME_, fl, 0, (k<TA_, 0>), grid, block, 0, s, P); }   \\\n    } while (0)\n'
            '    if (ta) GGAN_GEMM_CASE(true, "<true>");\n    else GGAN_GEMM_CASE(false, "<false>");\n#undef GGAN_GEMM_CASE\n'
            '#define GGAN_SKINNY_NS(NAME_) \\\n  if (ns == 1) { GGAN_LAUNCH("s" NAME_, fl, 0, (s<true, 1>), grid, dim3(512), 0, s, P); } \\\n'
            '  else { GGAN_LAUNCH("s" NAME_, fl, 0, (s<true, 8>), grid, dim3(512), 0, s, P); }\n    GGAN_SKINNY_NS("<a, b>");\n'
            '    GGAN_LAUNCH("plain_k", 2.0 * M, 0, plain_k, dim3(cdiv(M, 4)), dim3(256), 0, s, A);\n'
            '    GGAN_LAUNCH("grp<8>", 4.0 * M * K * (double)H, 0, grp<8>, dim3(nwg), dim3(512), 0, s, GG);\n')
    assert source_pairs(text) == {('k8<true>', 1), ('k8<false>', 1), ('k<true>', 0), ('k<false>', 0), ('s<a, b>', 1), ('s<a, b>', 8),
                                  ('plain_k', None), ('grp<8>', None)}


def test_every_launched_variant_has_a_row_and_every_row_a_launch():
    text = _read()
    src = source_pairs(text)
    kinds = (FF, FT, TF, TT, FT1, TF2)
    assert {p for p in src if p[0].startswith('gemm_kernel<')} == {('gemm_kernel' + k, f) for k in kinds for f in (0, 1, 2)}
    assert {p for p in src if p[0].startswith('gemm_kernel8<')} == {('gemm_kernel8' + k, f) for k in kinds for f in (1, 2)}
    assert {p for p in src if p[0].startswith('gemm_skinny_k')} == {('gemm_skinny_k' + k, n) for k in (FF, TF, TT) for n in (1, 2, 4, 8)}
    missing, stale = uncovered(text)
    assert not missing, 'launched by csrc/gemm.hip without a row in tests/_gemm_dispatch.py: %s' % missing
    assert not stale, 'rows of tests/_gemm_dispatch.py name what csrc/gemm.hip no longer launches: %s' % stale
    # the generic loader only in BIG_ROWS, the split-K reductions only ever as helpers
    assert all(r['expect'][0]['fast'] != 0 for r in ROWS) and all(r['expect'][0]['fast'] == 0 for r in BIG_ROWS)
    also = {a for r in ROWS for a in r['also']}
    assert REDUCES <= also and not (REDUCES & {r['kernel'] for r in ROWS + BIG_ROWS})
    # a helper named in `also` is launched by this file or is a split-K reduction (conv_corr.hip)
    assert also <= {p[0] for p in src} | REDUCES, sorted(also)


def test_a_scratch_copy_with_one_more_arm_is_caught():
    """one more FAST arm of gemm_kernel8, one more NS arm of the skinny kernel, one more launch site"""
    text = _read()
    arm = 'else if (w8) { GGAN_LAUNCH("gemm_kernel8" NAME_, fl, 0, (gemm_kernel8<TA_, TB_, MK_, 2>), grid, dim3(512), 0, s, P); }'
    assert text.count(arm) == 1
    text = text.replace(arm, arm + ' \\\n        else if (w8x) { GGAN_LAUNCH("gemm_kernel8" NAME_, fl, 0, (gemm_kernel8<TA_, TB_, MK_, 3>), grid, dim3(512), 0, s, P); }')
    arm = 'else if (ns == 4) { GGAN_LAUNCH("gemm_skinny_k" NAME_, fl, 0, (gemm_skinny_k<TB_, MK_, 4>), grid, dim3(512), 0, s, P); }'
    assert text.count(arm) == 1
    text = text.replace(arm, arm + ' \\\n            else if (ns == 16) { GGAN_LAUNCH("gemm_skinny_k" NAME_, fl, 0, (gemm_skinny_k<TB_, MK_, 16>), grid, dim3(512), 0, s, P); }')
    text += '    GGAN_LAUNCH("gemv_cols_k", 2.0 * N * K, 0, gemv_cols_k, dim3(cdiv(N, 4)), dim3(256), 0, s, A, B, C);\n'
    missing, stale = uncovered(text)
    kinds = (FF, FT, FT1, TF, TF2, TT)
    assert missing == sorted([('gemm_kernel8' + k, 3) for k in kinds] + [('gemm_skinny_k' + k, 16) for k in (FF, TF, TT)] + [('gemv_cols_k', None)],
                             key=lambda p: (p[0], -1 if p[1] is None else p[1])), missing
    assert stale == [], stale


def test_a_scratch_copy_with_one_arm_fewer_is_caught():
    """the generic-loader arm of gemm_kernel, the NS = 2 arm of the skinny kernel and the gemv launch removed"""
    text = _read()
    arm = 'else { GGAN_LAUNCH("gemm_kernel" NAME_, fl, 0, (gemm_kernel<TA_, TB_, MK_, 0>), grid, block, 0, s, P); }'
    assert text.count(arm) == 1
    text = text.replace(arm, '')
    arm = 'else if (ns == 2) { GGAN_LAUNCH("gemm_skinny_k" NAME_, fl, 0, (gemm_skinny_k<TB_, MK_, 2>), grid, dim3(512), 0, s, P); }'
    assert text.count(arm) == 1
    text = text.replace(arm, '')
    assert text.count('GGAN_LAUNCH("gemv_rows_k"') == 1
    text = text.replace('GGAN_LAUNCH("gemv_rows_k"', 'GGAN_LAUNCH_OFF("gemv_rows_k"')
    missing, stale = uncovered(text)
    assert missing == [], missing
    assert stale == sorted([('gemm_kernel' + k, 0) for k in (FF, FT, FT1, TF, TF2, TT)] + [('gemm_skinny_k' + k, 2) for k in (FF, TF, TT)]
                           + [('gemv_rows_k', None)], key=lambda p: (p[0], -1 if p[1] is None else p[1])), stale


# ---- the planner, transcribed -----------------------------------------------------------------------------------------------------------
BM = BN = 64
BK, KSTEP = 16, 32
WS_BYTES = (192 << 20) - 16384          # functional.workspace() less GGAN_WS_RESERVED
LIMIT = 0x7FFFFFF0


def cdiv(a, b):
    return -(-a // b)


def skinny(ta, tb, M, N, K, colsum=False, a_split=0, c_split=0, a_ref=False, b_ref=False):
    """gemm_launch's predicate for gemm_skinny_k"""
    tiles = cdiv(M, BM) * cdiv(N, BN)
    return (not ta and not colsum and (not a_split or (a_split % 16 == 0 and not a_ref)) and (not c_split or c_split % 16 == 0) and not b_ref
            and (not a_ref or bool(tb)) and M >= 32 and 64 <= K <= 1024 and tiles < 64 and cdiv(M, 16) * cdiv(N, 16) <= 1024
            and not (K <= 128 and tiles >= 32) and M * K * 4 < LIMIT and N * K * 4 < LIMIT)


def skinny_ns(K):
    steps = cdiv(cdiv(K, 16), 8)
    return 1 if steps <= 1 else 2 if steps <= 2 else 4 if steps <= 4 else 8


def gemm_plan(mode, ta, tb, M, N, K, colsum=False, a_split=0, c_split=0, al_a=True, al_a2=True, al_b=True, al_ref=True, a_ref=False,
              b_ref=False, sk_env=None, split_target=256, ws_bytes=WS_BYTES):
    """gemm_plan + gemm_launch_planned's choice of the eight-wave kernel -> dict(waves, fast, SK, kps, grid)"""
    lda, ldb, lda2 = (M if ta else K), (K if tb else N), 0
    if a_split:
        assert 0 < a_split < lda and a_split % 64 == 0 and not a_ref
        lda, lda2 = a_split, lda - a_split
    if c_split:
        assert 0 < c_split < N and c_split % BN == 0 and not colsum
    vec_a = al_a and lda % 4 == 0 and (not a_ref or al_ref) and (not a_split or (al_a2 and lda2 % 4 == 0))
    vec_b = al_b and ldb % 4 == 0 and (not b_ref or al_ref)
    gx, gy = cdiv(N, BN), cdiv(M, BM)
    sk = 1
    if mode == 0 and not c_split:
        if sk_env is not None:
            sk = sk_env
        else:
            base, tall = gx * gy, K >= 16384
            sk = min((1024 if tall else split_target) // base, K // BK, 256 if tall else split_target // 4)
            if K <= 128 and base >= 32:
                sk = 1
        sk = max(sk, 1)
        if colsum and not (gx * gy < 64 and K >= 512):
            sk = 1
        while sk > 1 and sk * (M * N + (N if colsum else 0)) * 4 > ws_bytes:
            sk //= 2
    kq = KSTEP if (a_split and not ta) else BK
    kps = cdiv(cdiv(K, sk), kq) * kq
    SK = cdiv(K, kps)
    size_a = (K * a_split if ta else M * a_split) * 4 if a_split else M * K * 4
    size_a2 = (K * (M - a_split) if ta else M * (K - a_split)) * 4 if a_split else 0
    dims4 = K % 4 == 0 and kps % 4 == 0 and (not ta or (M % 4 == 0 and a_split % 4 == 0)) and (bool(tb) or N % 4 == 0)
    small = size_a < LIMIT and size_a2 < LIMIT and N * K * 4 < LIMIT
    fast = 0 if not small else 1 if (vec_a and vec_b and dims4) else 2
    return dict(waves=8 if (fast != 0 and kps >= 2 * KSTEP) else 4, fast=fast, ns=0, SK=SK, kps=kps, grid=(gx, gy, SK))


def _kind(ta, tb, a_ref=False, b_ref=False):
    return FT1 if a_ref else TF2 if b_ref else (FF, FT, TF, TT)[2 * ta + tb]


def _reduce(SK, elems, tail=0):
    return () if SK == 1 else ('splitk_reduce_small_k',) if (SK >= 8 and elems + tail <= 65536) else ('splitk_reduce_k',)


def planned(row):
    """-> (kernel, expect tuple, also set, tail or None) the transcription derives for a row"""
    sk_env = int(row['env']['GGAN_GEMM_SK']) if 'GGAN_GEMM_SK' in row['env'] else None
    off = row['off']
    if row['entry'] in HEADS:
        M, K1, K2, H = row['shape']
        K = K1 + K2
        al_a1, al_a2, al_w = (o == 0 for o in off)
        if row['entry'] in ('critic_head_fwd', 'critic_head_fwd_bce'):
            p = gemm_plan(0, 0, 0, M, H, K, a_split=K1 if K2 else 0, al_a=al_a1, al_a2=al_a2, al_b=al_w, sk_env=sk_env, split_target=512)
            name = 'head_out_fwd_k' if row['entry'] == 'critic_head_fwd' else 'head_out_fwd_bce_k'
            return name, (dict(waves=4, fast=-1, ns=0, SK=p['SK'], kps=p['kps'], grid=(cdiv(M, 2), 1, 1)),), \
                {('gemm_kernel8' if p['waves'] == 8 else 'gemm_kernel') + FF}, None
        with_tail = row['entry'] == 'critic_head_bwd_tail'
        also = set() if with_tail else {'head_out_bwd_k'}
        pw = gemm_plan(1, 1, 0, K, H, M, colsum=True, a_split=K1 if K2 else 0, al_a=al_a1, al_a2=al_a2) if row['need'] == 'all' else None
        pa = gemm_plan(1, 0, 1, M, K, H, c_split=K1 if K2 else 0, al_b=al_w)
        na = pa['grid'][0] * pa['grid'][1]
        nt = 1 + cdiv(H, 16)
        if pw and pw['fast'] == 1 and pa['fast'] == 1:
            nw = pw['grid'][0] * pw['grid'][1]
            return 'gemm_group_kernel<8>', (dict(pa, waves=8, wgs=(0, na)), dict(pw, waves=8, wgs=(na, na + nw))), also, \
                (na + nw, na + nw + nt) if with_tail else None
        if with_tail and not pw and pa['fast'] == 1:
            return 'gemm_group_kernel<8>', (dict(pa, waves=8, wgs=(0, na)),), also, (na, na + nt)
        name = lambda p, k: ('gemm_kernel8' if p['waves'] == 8 else 'gemm_kernel') + k
        if with_tail:
            also.add('head_tail_k')
        launched = ([(name(pw, TF), pw)] if pw else []) + [(name(pa, FT), pa)]
        main = [x for x in launched if x[0] == row['kernel']]
        assert len(main) == 1, (row, launched)
        return row['kernel'], (main[0][1],), also | {n for n, _ in launched if n != row['kernel']}, None
    ta, tb, M, N, K = row['shape']
    colsum = row['entry'] in ('gemm_colsum', 'linear_bwd_weight_act') or bool(row.get('colsum'))
    a_ref, b_ref = row['entry'] == 'linear_bwd_data_act' and bool(row['mask']), row['entry'] == 'linear_bwd_weight_act' and bool(row['mask'])
    if N == 1 and not ta and not tb and not colsum and not a_ref and not b_ref:
        return 'gemv_rows_k', (dict(waves=4, fast=-1, ns=0, SK=1, kps=K, grid=(cdiv(M, 4), 1, 1)),), set(), None
    if skinny(ta, tb, M, N, K, colsum, row['a_split'], row['c_split'], a_ref, b_ref):
        return 'gemm_skinny_k' + (TT if a_ref else TF if tb else FF), \
            (dict(waves=8, fast=-1, ns=skinny_ns(K), SK=1, kps=K, grid=(cdiv(N, 16), cdiv(M, 16), 1)),), set(), None
    p = gemm_plan(0, ta, tb, M, N, K, colsum=colsum, a_split=row['a_split'], c_split=row['c_split'], al_a=off[0] == 0, al_a2=off[1] == 0,
                  al_b=off[2] == 0, al_ref=off[3] == 0, a_ref=a_ref, b_ref=b_ref, sk_env=sk_env)
    return ('gemm_kernel8' if p['waves'] == 8 else 'gemm_kernel') + _kind(ta, tb, a_ref, b_ref), (p,), \
        set(_reduce(p['SK'], M * N, N if colsum else 0)), None


def test_recorded_plans_follow_the_planner():
    for r in ROWS + BIG_ROWS:
        kernel, expect, also, tail = planned(r)
        assert kernel == r['kernel'], (row_id(r), kernel)
        assert expect == r['expect'], (row_id(r), expect, r['expect'])
        assert also == set(r['also']), (row_id(r), also)
        assert tail == r.get('tail'), (row_id(r), tail)


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS + BIG_ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for r in ROWS + BIG_ROWS:
        assert r['entry'] in ENTRIES and set(r['env']) <= {'GGAN_GEMM_SK'}, r
        assert r['act'] in ('none', 'lrelu', 'relu') and r['mask'] in (None, 'lrelu', 'relu'), r
        assert all(0 <= o <= 3 for o in r['off']) and len(r['off']) == (3 if r['entry'] in HEADS else 4), r
        assert bool(r['mask']) == (r['entry'] in ('linear_bwd_data_act', 'linear_bwd_weight_act')), r
        for x in r['expect']:
            assert x['waves'] in (4, 8) and x['kps'] >= 1 and x['SK'] >= 1 and x['grid'][2] in (1, x['SK']), r
    for r in ROWS:
        if r['entry'] in HEADS:
            M, K1, K2, H = r['shape']
            assert M * max(K1 + K2, H) <= 2 ** 20 and K1 + K2 <= 4608 and H % 4 == 0, r
            if 'terms' in r:
                assert sum(t[0] for t in r['terms']) == M, r
        else:
            ta, tb, M, N, K = r['shape']
            assert K <= 4608 and M * N <= 2 ** 20 and 2.0 * M * N * K <= 2e9, r          # well under a second each
            assert r['entry'] != 'gemm' or (not r['a_split'] and not r['c_split']), r
            assert not (r['bias'] or r['act'] != 'none') or r['entry'] in ('gemm', 'gemm_split'), r
    for r in BIG_ROWS:
        ta, tb, M, N, K = r['shape']
        big = {'A': M * (r['a_split'] or K), 'B': N * K}[r['big']] * 4
        assert big >= LIMIT and r['along'] in ('M', 'N', 'K') and dict(M=M, N=N, K=K)[r['along']] % r['reps'] == 0, r
        assert K <= 2 ** 24 and max(r['expect'][0]['grid'][1:]) <= 65535, r


def test_table_keeps_the_cases_it_was_written_for():
    x0 = lambda r: r['expect'][0]
    tile = [r for r in ROWS if r['kernel'].startswith('gemm_kernel') and r['entry'] not in HEADS]
    steps = lambda r: x0(r)['kps'] / KSTEP
    last = lambda r: r['shape'][4] - (x0(r)['SK'] - 1) * x0(r)['kps']
    for name, waves in (('gemm_kernel<', 4), ('gemm_kernel8<', 8)):
        rows = [r for r in tile if r['kernel'].startswith(name)]
        assert all(x0(r)['waves'] == waves for r in rows)
        # steps per split: the four-wave kernel is only ever planned with kps < 2 * KSTEP on the buffer-load paths (1, 2 half-empty);
        # its 3- and 4-step splits are generic-loader rows
        pool = rows + ([r for r in BIG_ROWS] if waves == 4 else [])
        have = {steps(r) for r in pool} | {last(r) / KSTEP for r in pool if x0(r)['SK'] > 1}
        assert {1, 2, 3, 4} <= {int(-(-s // 1)) for s in have}, (name, sorted(have))
        assert any(x0(r)['SK'] == 1 for r in rows) and any(x0(r)['SK'] > 1 for r in rows), name
        assert any(x0(r)['SK'] > 1 and last(r) < x0(r)['kps'] for r in rows), name                     # a shorter last split
        assert any(last(r) % KSTEP for r in rows), name                                              # K % KSTEP != 0 in the last split
        for fast in (1, 2):
            for mask in (FT1, TF2):
                assert any(r['kernel'] == name[:-1] + mask and x0(r)['fast'] == fast for r in rows), (name, mask, fast)
        # FAST 2: once by a leading dimension, once by a base offset with every dimension a multiple of 4 -- for A and for B
        f2 = [r for r in rows if x0(r)['fast'] == 2]
        by_off = lambda i: any(r['off'][i] and not any(d % 4 for d in r['shape'][2:]) for r in f2)
        assert by_off(0) and by_off(2), name
        ld_a = lambda r: r['shape'][2] if r['shape'][0] else r['shape'][4]
        ld_b = lambda r: r['shape'][4] if r['shape'][1] else r['shape'][3]
        assert any(not any(r['off']) and ld_a(r) % 4 for r in f2) and any(not any(r['off']) and ld_b(r) % 4 for r in f2), name
    assert any(x0(r)['kps'] == 16 for r in tile) and any(x0(r)['kps'] == 48 for r in tile)
    # column sums: unsplit, split with the slab tail, with the mask on B
    cs = [r for r in tile if r['entry'] in ('gemm_colsum', 'linear_bwd_weight_act') or r.get('colsum')]
    assert any(x0(r)['SK'] == 1 for r in cs) and any(x0(r)['SK'] > 1 and r['entry'] == 'gemm_colsum' for r in cs)
    assert any(x0(r)['SK'] > 1 and r['kernel'].endswith(TF2) for r in cs) and any(x0(r)['SK'] == 1 and r['kernel'].endswith(TF2) for r in cs)
    # two-source operand and split output, in the tile kernels and in the skinny kernel
    two = [r for r in ROWS if r['a_split'] and r['entry'] == 'gemm_split']
    assert any(not r['shape'][0] and r['shape'][4] - r['a_split'] < KSTEP for r in two if r in tile)      # sources split k
    assert any(r['shape'][0] and r['shape'][2] - r['a_split'] < BM for r in two if r in tile)             # sources split m
    sk_two = [r for r in two if r['kernel'].startswith('gemm_skinny_k')]
    assert any(r['a_split'] % 16 == 0 and r['a_split'] % 64 for r in sk_two) and any((r['shape'][4] - r['a_split']) % 4 for r in sk_two)
    outs = [r for r in ROWS if r['c_split']]
    assert any(r in tile for r in outs) and any(r['kernel'].startswith('gemm_skinny_k') for r in outs)
    # the skinny kernel: alignment, masks, the predicate's boundaries on both sides
    sk = [r for r in ROWS if r['kernel'].startswith('gemm_skinny_k')]
    assert any(r['off'][0] and r['shape'][4] % 4 == 0 for r in sk) and any(r['off'][2] and r['shape'][4] % 4 == 0 and r['shape'][1] for r in sk)
    assert {r['mask'] for r in sk if r['kernel'].endswith(TT)} == {'lrelu', 'relu'}
    plain = [r for r in ROWS if r['entry'] == 'gemm' and not r['shape'][0]]
    side = lambda cond: {r['kernel'].startswith('gemm_skinny_k') for r in plain if cond(r['shape'])}
    assert side(lambda s: s[2] == 32) == {True} and side(lambda s: s[2] == 31) == {False}
    assert side(lambda s: s[4] == 64) == {True} and side(lambda s: s[4] == 63) == {False}
    assert side(lambda s: s[4] == 1024) == {True} and side(lambda s: s[4] == 1040) == {False}
    # (cdiv(M, 16) * cdiv(N, 16) <= 1024 can never decide: fewer than 64 tiles of 64 x 64 hold at most 63 * 16 = 1008 of 16 x 16)
    tiles = lambda s: cdiv(s[2], 64) * cdiv(s[3], 64)
    assert side(lambda s: tiles(s) == 63) == {True} and side(lambda s: tiles(s) == 64) == {False}
    assert side(lambda s: s[4] <= 128 and tiles(s) >= 32) == {False} and True in side(lambda s: s[4] == 128 and 16 <= tiles(s) < 32)
    # group launches and the heads' separate launches
    grp = [r for r in ROWS if r['kernel'] == 'gemm_group_kernel<8>']
    assert sorted((len(r['expect']), 'tail' in r) for r in grp) == [(1, True), (2, False), (2, True)]
    sep = [r for r in ROWS if r['entry'] in ('critic_head_bwd', 'critic_head_bwd_tail') and r not in grp]
    assert {('head_tail_k' in r['also']) for r in sep} == {True, False} and all(x0(r)['fast'] == 2 for r in sep)
    assert {r['entry'] for r in ROWS} == set(ENTRIES)
    assert any(r['kernel'] == 'gemv_rows_k' for r in ROWS)
    # the generic loader: every kind with A large, B large, a second source beyond 2^31 bytes
    assert {r['kernel'] for r in BIG_ROWS if r['big'] == 'A' and not r['a_split']} == {'gemm_kernel' + k for k in (FF, FT, TF, TT, FT1, TF2)}
    assert any(r['big'] == 'B' for r in BIG_ROWS)
    assert any(r['a_split'] and r['shape'][2] * r['a_split'] * 4 > 2 ** 31 for r in BIG_ROWS)


# ---- the exact data of the generic-loader rows --------------------------------------------------------------------------------------------
def test_big_row_data_is_exact_and_shows_every_displacement():
    """The construction test_gemm_dispatch_gpu.py uses, at a reduced repeat count: the dense float64 product of the materialised operands
    equals the reference computed from the generating blocks, and reading any one copy of the large operand from the copy before it
    changes the result.  At the rows' own size: every output element sums fewer than 2^23 non-zero products, each a multiple of 1/2, so
    every partial sum in any order is exact in fp32; copies one apart, and 2^31 / 2^32 bytes apart where that is a whole number of
    copies, carry different multipliers."""
    fars = []
    for r in BIG_ROWS:
        ta, tb, M, N, K = r['shape']
        reps = 12
        small = dict(r, shape=(ta, tb) + tuple(96 * reps if n == r['along'] else v for n, v in zip('MNK', (M, N, K))), reps=reps)   # 96-long copies
        d = D.big_operands(small, np.random.default_rng(5))
        ref, bound = D.big_reference(small, d), D.big_bound(small, d)
        dense = D.big_dense(small, d)
        assert set(dense) == set(ref)
        for what in ref:
            assert np.array_equal(dense[what], ref[what]), (row_id(r), what)
            assert np.array_equal(2 * ref[what], np.round(2 * ref[what])) and np.abs(ref[what]).max() <= bound, (row_id(r), what)
            assert np.abs(ref[what]).max() > 0
        for rep in range(1, reps):
            moved = D.big_dense(small, d, displaced=(rep, 1))
            assert not np.array_equal(moved['C'], ref['C']), (row_id(r), rep)
        # the row's own size: the bound on non-zero products (only the blocks and multipliers are needed), the far copies
        full = D.big_bound(r, D.big_operands(r, np.random.default_rng(5)))
        assert full < 2 ** 23, (row_id(r), full)
        mult = D.multipliers(r['reps'], np.random.default_rng(5))
        bb = D.big_block_bytes(r)
        far = [w // bb for w in (2 ** 31, 2 ** 32) if w % bb == 0 and w // bb < r['reps']]
        for dist in [1] + far:
            assert np.all(mult[dist:] != mult[:-dist]), (row_id(r), dist)
        fars.append((r['along'], far))
    # copies 2^31 bytes apart are checked for an operand stored along M, along K and along N, copies 2^32 bytes apart for the 4.5 GiB A
    assert {along for along, far in fars if far} == {'M', 'K', 'N'} and any(len(far) == 2 for _, far in fars)
