"""The coverage table tests/_scan_dispatch.py against csrc/dynscan.hip, without a GPU: the two GGAN_LAUNCH labels have rows and the rows
name no other; MAXD, H and the grid are the source's; the rows hold every edge they were built for; the float32 restatement of both
kernels passes every stage's bound on every row, against the layer-by-layer recurrence of oracle-style float64 too; each of eight wrong
kernels misses a bound by more than a factor of two on the row MUTANT_ROW names; the argument checks answer before any launch."""
import os
import re

import numpy as np

import _scan_dispatch as D
from _scan_dispatch import ROWS, row_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    return open(os.path.join(ROOT, 'graphical_gan_amd', 'csrc', 'dynscan.hip')).read()


def labels(text):
    out = re.findall(r'GGAN_LAUNCH\(\s*"([^"]+)"', text)
    assert len(out) == text.count('GGAN_LAUNCH(')
    return out


def uncovered(text, rows=ROWS):
    have, named = set(labels(text)), {l[0] for r in rows for l in r['launches']}
    return sorted(have - named), sorted(named - have)


def test_every_site_has_a_row_and_every_row_a_site():
    text = _source()
    assert labels(text) == ['dyn_scan_fwd_k', 'dyn_scan_bwd_k'] and uncovered(text) == ([], [])
    assert uncovered(text.replace('"dyn_scan_bwd_k"', '"dyn_scan_bwd2_k"')) == (['dyn_scan_bwd2_k'], ['dyn_scan_bwd_k'])
    assert uncovered(text, [r for r in ROWS if r['bwd_only']]) == (['dyn_scan_fwd_k'], [])


def test_transcribed_constants_are_the_sources():
    text = _source()
    assert 'constexpr int H = %d;' % D.H in text and 'constexpr int MAXD = %d;' % D.MAXD in text
    assert text.count('dim3(B), dim3(H), 0, (hipStream_t)stream, P);') == 2 and D.K_THREADS == D.H
    assert text.count('dl > 0 && dl <= MAXD && dt > 0 && dt <= MAXD && Hdim == H') == 2
    assert 'GGAN_CHECK_ARG((zw == nullptr) == (b_zw == nullptr), "zw and b_zw go together");' in text
    assert 'GGAN_CHECK_ARG((((uintptr_t)w_1 | (uintptr_t)w_in) & 15) == 0, "w_1 / w_in must be 16-byte aligned");' in text
    assert '__device__ __forceinline__ float lrelu(float v, float a) { return fmaxf(a * v, v); }' in text
    assert text.count('> 0.f ? 1.f : P.alpha') == 2                                       # the backward's masks, as check() restates them
    assert 'for (int k = 0; k < H; k += 8) {' in text and '((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])) + b1;' in text
    assert '((red[0][n] + red[1][n]) + (red[2][n] + red[3][n])) + P.b_out[n];' in text
    ops = open(os.path.join(ROOT, 'tests', 'test_ops_gpu.py')).read()                     # the weight scales are test_dyn_scan's
    for k, sc in (('w_in', 0.3), ('w_1', 0.08), ('w_out', 0.08), ('zw', 0.3)):
        assert D.SCALES[k] == sc and 'sc=%s)' % sc in ops


def test_rows_hold_their_edges():
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids)
    for r in ROWS:
        assert D.planned(r) == r['launches'] and r['note'], row_id(r)
        assert 1 <= r['dl'] <= D.MAXD and 1 <= r['dt'] <= D.MAXD
    both = (('dyn_scan_fwd_k', 1, (3,), (256,)), ('dyn_scan_bwd_k', 1, (3,), (256,)))
    assert D.by_id('B3-T2-dl16-dt16-res')['launches'] == both and D.by_id('B4-T3-dl6-dt4-res-bwd')['launches'] == (('dyn_scan_bwd_k', 1, (4,), (256,)),)
    shapes = {(r['B'], r['T'], r['dl'], r['dt'], r['mode']) for r in ROWS if not r['bwd_only']}
    assert shapes == {(1, 1, 1, 1, 'res'), (3, 2, 16, 16, 'res'), (3, 2, 16, 16, 'res_w'), (2, 3, 16, 1, 'res'), (2, 3, 1, 16, 'res_w'),
                      (5, 4, 8, 8, 'res_w'), (3, 30, 8, 8, 'res'), (33, 2, 4, 6, 'res_w')}
    assert {(r['dl'], r['dt']) for r in ROWS} >= set(D.ACCEPTED_SHAPES)
    assert sum(r['null'] for r in ROWS) == 2 and {r['mode'] for r in ROWS if r['null']} == {'res', 'res_w'}
    back = [(i, r) for i, r in enumerate(ROWS) if r['bwd_only']]
    assert {r['mode'] for _, r in back} == {'res', 'res_w'}
    for i, r in back:
        d = D.inputs(r, 8000 + i)
        for k in ('h1', 'h2'):
            z = d[k] == 0
            assert 0.05 < z.mean() < 0.2 and np.any(np.signbit(d[k][z])) and np.any(~np.signbit(d[k][z])), (row_id(r), k)
    assert all(D.offset(k) == 0 for k in D.ALIGNED) and all(D.offset(k) == 1 for k in D.INPUTS + D.FWD_OUT + D.BWD_OUT if k not in D.ALIGNED)


def _recurrence64(row, d):
    """the layer-by-layer recurrence, float64 -> zs [B, T + 1, dl]"""
    lre = lambda v: np.maximum(0.2 * v, v)
    W = {k: (np.asarray(v, np.float64) if v is not None else None) for k, v in d.items()}
    zs = [W['z0']]
    for _ in range(row['T']):
        h = lre(np.concatenate([zs[-1], W['eps']], 1) @ W['w_in'] + W['b_in'])
        h = lre(h @ W['w_1'] + W['b_1'])
        o = h @ W['w_out'] + W['b_out']
        zs.append(o + (zs[-1] @ W['zw'] + W['b_zw'] if row['mode'] == 'res_w' else zs[-1]))
    return np.stack(zs, 1)


def test_a_float32_restatement_of_both_kernels_passes_every_bound():
    worst = {}
    for idx, r in enumerate(ROWS):
        d = D.inputs(r, 8000 + idx)
        out = D.run32(r, d)
        fr = D.check(r, d, out)
        assert D.within(fr), (row_id(r), fr)
        for k, f in fr.items():
            worst[k] = max(worst.get(k, 0.0), f)
        if not r['bwd_only']:                          # the restatement is the operator: the whole sequence, as test_dyn_scan measures it
            ref = _recurrence64(r, d)
            assert np.abs(out['zs'] - ref).max() / np.abs(ref).max() < 1e-5, row_id(r)
    print('float32 restatement, worst fraction of the bound per stage:', {k: round(v, 3) for k, v in worst.items()})
    assert all(worst[k] > 0.02 for k in ('h1', 'h2', 'zs', 'G1', 'G2', 'Go', 'd_z0', 'd_eps')), worst          # no bound resolves nothing


def test_every_wrong_kernel_is_caught_on_its_row():
    index = {row_id(r): i for i, r in enumerate(ROWS)}
    assert len(D.MUTANTS) == 8
    for name, rid in D.MUTANT_ROW.items():
        idx = index[rid]
        d = D.inputs(ROWS[idx], 8000 + idx)
        wrong = D.check(ROWS[idx], d, D.run32(ROWS[idx], d, mutant=name))
        print('%-28s %-28s %s' % (name, rid, {k: v for k, v in wrong.items() if v > 1}))
        assert max(wrong.values()) > 2.0, 'a kernel with "%s" would pass %s' % (name, rid)
    # one wrong ELEMENT of one step, which a norm over the sequence hides at 1e-5 (one of 744 values off by 1e-4 of itself), and only it
    idx = index['B3-T30-dl8-dt8-res']
    d = D.inputs(ROWS[idx], 8000 + idx)
    out = D.run32(ROWS[idx], d)
    ref = out['zs'].copy()
    out['zs'][1, 17, 3] *= np.float32(1.0001)
    assert np.abs(out['zs'] - ref).max() / np.abs(ref).max() < 1e-5
    fr = D.check(ROWS[idx], d, out)
    assert fr['zs'] > 2.0 and all(fr[k] <= 1.0 for k in ('h2', 'G1', 'G2', 'Go', 'd_z0', 'd_eps')), fr          # (h1[17] and Xin[17] read the element)


def test_a_nan_in_any_output_fails():
    idx = 2
    d = D.inputs(ROWS[idx], 8000 + idx)
    good = D.run32(ROWS[idx], d)
    for key in good:
        out = {k: v.copy() for k, v in good.items()}
        out[key].flat[out[key].size - 1] = np.nan
        fr = D.check(ROWS[idx], d, out)
        assert not D.within(fr) and not any(np.isnan(f) for f in fr.values()), (key, fr)


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    pointer = lambda k: (k + 1) << 24           # (never dereferenced: every case fails its checks first)
    for case in D.REJECTED:
        rc, msg = D.call(L, case, pointer)
        assert rc != 0 and case[0] + ':' in msg and case[2] in msg, (case, rc, msg)
    words = {(c[0], c[2]) for c in D.REJECTED}
    assert ('ggan_dyn_scan_fwd', 'zw and b_zw go together') in words and ('ggan_dyn_scan_bwd', '16-byte aligned') in words
    assert any(c[0] == 'ggan_dyn_scan_fwd' and c[1][2] == 17 for c in D.REJECTED) and any(c[1][3] == 0 for c in D.REJECTED)
    assert any(c[1][4] == 128 for c in D.REJECTED)
