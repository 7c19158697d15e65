"""The coverage table tests/_latent_dispatch.py against csrc/latent.hip, without a GPU: every GGAN_LAUNCH label and every kernel instance
of latent.hip has a row and the rows name nothing else; the constants planned() and the host Philox copy are the source's; every row's
launches follow from planned(); the rows reach every edge the table promises; Philox4x32-10 gives the known answers and the extreme seeds
give their words; the float32 restatement of the kernels (run32) passes every bound on every row, while each wrong kernel of MUTANTS
misses a bound or breaks an exact stage on the row named here; and the calls of REJECTED answer before any launch."""
import os
import re

import numpy as np
import pytest

import _latent_dispatch as D
from _latent_dispatch import ROWS, row_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 9000


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _source():
    return _read('graphical_gan_amd', 'csrc', 'latent.hip')


_LAUNCH = re.compile(r'GGAN_LAUNCH\(\s*"([^"]+)"\s*,.*?,\s*(\w+_k(?:<\w+>)?)\s*,\s*dim3\(([^;]*?)\),\s*dim3\((\w+)\),\s*(.*?),\s*\(hipStream_t\)', re.S)


def sites(text):
    """-> {(label, kernel instance)} of every GGAN_LAUNCH site of the text"""
    found = list(_LAUNCH.finditer(text))
    assert len(found) == text.count('GGAN_LAUNCH('), (len(found), text.count('GGAN_LAUNCH('))
    return {(s.group(1), s.group(2)) for s in found}


def row_sites(rows):
    return {(l[0], l[4]) for r in rows for l in r['launches']}


_INPUTS = {}


def _inp(i):
    if i not in _INPUTS:
        _INPUTS[i] = D.inputs(ROWS[i], SEED + i)
    return _INPUTS[i]


def _index(rid):
    return [row_id(r) for r in ROWS].index(rid)


def _of(e, **kw):
    return [r for r in ROWS if r['entry'] == e and all(r[k] == v for k, v in kw.items())]


# ---- launch sites, kernels, constants, the plan -------------------------------------------------------------------------------------------
def test_every_site_and_kernel_instance_has_a_row_and_every_row_a_site():
    text = _source()
    assert sites(text) == row_sites(ROWS), (sorted(sites(text) - row_sites(ROWS)), sorted(row_sites(ROWS) - sites(text)))
    assert len(sites(text)) == 9 and len({l for l, _ in sites(text)}) == 9
    kernels = D.source_kernels(text)
    assert len(kernels) == 8 and kernels == sorted({k.split('<')[0] for _, k in row_sites(ROWS)}), kernels
    assert {k for _, k in row_sites(ROWS) if '<' in k} == {'gmm_latent_st_fwd_k<kModeKStc>', 'gmm_latent_st_fwd_k<kModeKSt>'}
    assert len(re.findall(r'^int ggan_\w+\(', text, flags=re.M)) == 8          # (the exported entry points of this unit)
    assert {k for r in ROWS for k in D.kernels_of(r).values()} <= set(kernels)
    # dynamic LDS as written at each site
    lds = {s.group(2): s.group(5).strip() for s in _LAUNCH.finditer(text)}
    assert {k for k, v in lds.items() if v != '0'} == {'gmm_posterior_assign_k', 'cluster_accuracy_k'}
    assert lds['gmm_posterior_assign_k'] == '(size_t)K * sizeof(float)' and lds['cluster_accuracy_k'] == '(size_t)K * sizeof(int)'
    for r in ROWS:
        for l in r['launches']:
            assert l[5] == (4 * r['K'] if lds[l[4]] != '0' else 0), (row_id(r), l)
    assert all(s.group(4) == '256' for s in _LAUNCH.finditer(text))


def test_a_scratch_copy_with_a_new_or_a_lost_site_is_caught():
    text = _source()
    site = 'GGAN_LAUNCH("mix_mean"'
    assert text.count(site) == 1
    assert ('mix_mean2', 'mix_mean_k') in sites(text.replace(site, 'GGAN_LAUNCH("mix_mean2"')) - row_sites(ROWS)
    assert ('mix_mean', 'mix_mean_k') in sites(text) - row_sites([r for r in ROWS if r['entry'] != 'mix'])
    assert ('gmm_latent_st_fwd', 'gmm_latent_st_fwd_k<kModeKSt>') in sites(text) - {s for s in row_sites(ROWS) if 'kModeKSt>' not in s[1]}


def test_transcribed_constants_are_the_sources():
    text, hdr = _source(), _read('include', 'ggan.h')
    assert 'constexpr int kGmmMaxK = %d;' % D.GMM_MAX_K in text and '#define GGAN_NOISE_MAX %d' % D.NOISE_MAX in hdr
    assert '#define GGAN_POSTERIOR_MAX_K %d' % D.POSTERIOR_MAX_K in hdr
    assert 'enum { GGAN_MODE_K_CONCRETE = 0, GGAN_MODE_K_STC = %d, GGAN_MODE_K_ST = %d };' % (D.MODE_STC, D.MODE_ST) in hdr
    for c in (D.PHILOX_M0, D.PHILOX_M1, D.PHILOX_W0, D.PHILOX_W1):
        assert '0x%08Xu' % c in text
    assert '__umulhi(0x%08Xu, c0)' % D.PHILOX_M0 in text and '__umulhi(0x%08Xu, c2)' % D.PHILOX_M1 in text
    assert 'k0 += 0x%08Xu; k1 += 0x%08Xu;' % (D.PHILOX_W0, D.PHILOX_W1) in text and 'for (int r = 0; r < 10; ++r)' in text
    assert 'cdivz(mx, (size_t)%d)' % D.NOISE_PER_WG in text and 'if (gx > %d) gx = %d;' % (D.NOISE_GRID_CAP, D.NOISE_GRID_CAP) in text
    assert 'if (gx < 1) gx = 1;' in text and 'dim3(gx, count)' in text
    assert 'sincosf(6.28318530718f * u01' in text and '+ 1e-20f) + 1e-20f)' in text
    assert 'fminf(((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f), 0.99999994f)' in text and np.float32(0.99999994) == D.U01_MAX
    assert '(unsigned)ti | 0x80000000u' in text and 'sizes[i] < 0x7FFFFFFFull' in text
    assert D.BIG_N == D.NOISE_GRID_CAP * D.NOISE_PER_WG + 1027 and 4 * D.BIG_N < 1.1e6
    build = _read('graphical_gan_amd', 'build.py')
    assert "'-ffp-contract=on'" in build and 'fast-math' not in build                        # what the rounding counts assume


def test_the_documented_interval_of_the_uniform_kind_is_what_the_rows_assert():
    hdr, ops, text = _read('include', 'ggan.h'), _read('graphical_gan_amd', 'functional', 'optim_ops.py'), _source()
    for t in (hdr, ops, text):
        assert '[a, b)' not in t.replace('[a, b) for a = 0', '')
    assert '1 = uniform on (a, b) for a = 0 and on [a, b] otherwise' in hdr
    assert '(a, b) for a = 0, [a, b] otherwise' in ops


def test_recorded_launches_follow_the_dispatch():
    for r in ROWS:
        assert D.planned(r) == r['launches'], (row_id(r), D.planned(r), r['launches'])
        assert all(len(l) == 6 and l[1] >= 1 for l in r['launches']) and r['note']
    ids = [row_id(r) for r in ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    big = _of('noise', seed=11)[0]
    assert big['launches'] == (('noise_fill', 1, (256, 2), (256,), 'noise_fill_k', 0),) and 'about 1 MB' in big['note']
    assert _of('noise', seed=12)[0]['launches'][0][2] == (1, 16) and ROWS[0]['launches'][0][2] == (2, 12)
    assert _of('latent', B=5, K=256)[0]['launches'][-1][2] in ((5,), (261,))


# ---- the edges, from the rows ---------------------------------------------------------------------------------------------------------------
def test_noise_rows_reach_every_edge():
    noise = _of('noise')
    sizes = {(s[0], s[1]) for r in noise for s in r['specs']}
    for kind in (D.UNIFORM, D.NORMAL):
        assert {n for k, n in sizes if k == kind} >= {1, 2, 3, 5, 1027} or kind == D.NORMAL
    assert {n for _, n in sizes} >= {1, 2, 3, 5, 1027, D.BIG_N} and D.BIG_N % 4 == 3 and D.BIG_N > D.NOISE_GRID_CAP * D.NOISE_PER_WG
    assert {s[4] for r in noise for s in r['specs'] if s[0] == D.ONEHOT} == {1, 3, 30, 256}
    assert any(s[0] == D.ONEHOT and s[4] == 3 and s[1] > 4 for s in ROWS[0]['specs'])        # rows straddle the groups of 4
    assert {(s[2], s[3]) for r in noise for s in r['specs'] if s[0] == D.UNIFORM} == {(0.0, 1.0), (0.0, 1.0 / 128), (-1.0, 3.0), (1.0, 2.0)}
    assert max(len(r['specs']) for r in noise) == D.NOISE_MAX and any(r['seed'] >> 32 for r in noise)
    assert any(r['draws'] == (2 ** 32 - 1, None) for r in noise) and any(r['draws'][:2] == (7, 7) for r in noise)
    assert {r['seed'] for r in noise} >= set(D.EXTREME_SEEDS)
    for seed, (onehot, w, word) in D.EXTREME_SEEDS.items():
        for r in _of('noise', seed=seed):
            assert r['draws'] == (0,) and len(r['specs']) == 1 and (r['specs'][0][0] == D.ONEHOT) == onehot


def test_latent_mix_and_posterior_rows_reach_every_edge():
    lat = _of('latent')
    assert {r['D'] for r in lat} == {1, 63, 65, 130, 257, 300} and {r['K'] for r in lat} >= {1, 4, 5, 255, 256}
    assert {r['B'] for r in lat if r['bwd']} == {1, 5, 255, 256} and {r['B'] for r in lat if not r['bwd']} == {300}
    assert {r['D'] for r in lat if r['bwd']} >= {257, 300} and {r['temp'] for r in lat} == {1.0, 0.5, 0.1}
    assert {(r['gl'], r['gk'], r['dz'], r['dmu']) for r in lat if r['bwd']} == \
        {(a, b, c, d) for a, b in ((1, 1), (1, 0), (0, 1)) for c, d in ((1, 1), (1, 0), (0, 1))}
    assert sum(r['u_one'] for r in lat) == 1
    assert all(r['B'] <= D.GMM_MAX_K or not r['bwd'] for r in lat) and all(r['K'] <= D.GMM_MAX_K for r in lat)
    mix = _of('mix')
    assert {r['B'] * r['D'] // 4 for r in mix} == {255, 256, 257} and {r['K'] for r in mix} == {1, 30, 100}
    assert {r['onehot'] for r in mix} == {True, False} and all(r['D'] % 4 == 0 for r in mix)
    post = _of('post')
    assert {r['K'] for r in post} == {1, 255, 257, 300, D.POSTERIOR_MAX_K} and {r['D'] for r in post} == {1, 65, 130}
    assert any(r['batches'] == ((0, 1),) for r in post)
    assert all([r0 for r0, _ in r['batches']] == [128, 0, 64] for r in post if len(r['batches']) > 1) and sum(len(r['batches']) > 1 for r in post) >= 4
    acc = _of('acc')[0]
    i = _inp(ROWS.index(acc))
    assert acc['N'] == 300 and -1 in i['assign'] and acc['K'] in i['assign'] and i['colbest'][0] == 0 and i['colbest'][1] == 0xFFFFFFFF
    assert 0 in i['assign'] and 1 in i['assign'] and (0xFFFFFFFF - int(i['colbest'][-1] & np.uint64(0xFFFFFFFF))) >= acc['N']
    assert max(4 * max(s[1] for s in r['specs']) for r in _of('noise')) == 4 * D.BIG_N                  # nothing larger than the 1 MB row
    assert all(4 * r['K'] * max(b for _, b in r['batches']) < 4 * D.BIG_N for r in post)


def test_inputs_are_what_the_rows_promise():
    for idx, r in enumerate(ROWS):
        if r['entry'] != 'latent':
            continue
        inp = _inp(idx)
        m = D.margins(r, inp)
        assert all(v.shape == (r['B'],) and np.all(v > 0) for v in m.values()), row_id(r)      # every row: none is left out
        u = inp['u']
        assert np.all(u >= np.float32(2.0 ** -25)) and (np.all(u <= D.U01_MAX) or r['u_one'])
        want = [np.float32(2.0 ** -25), np.float32(0.5), D.U01_MAX][:r['B'] * r['K']] + ([np.float32(1.0)] if r['u_one'] else [])
        assert r['B'] * r['K'] < 3 or all(np.any(u == w) for w in want), row_id(r)
        if r['K'] >= 2:
            j1, j2 = D.tie_pair(r['K'])
            assert j1 < j2 and np.array_equal(inp['mu'][j1].view(np.uint32), inp['mu'][j2].view(np.uint32)) and u[0, j1] == u[0, j2]
            assert np.array_equal(inp['z'][0].view(np.uint32), inp['mu'][j1].view(np.uint32))
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'post' and len(r['batches']) > 1:
            zs = _inp(idx)['zs']
            assert np.array_equal(zs[0][1].view(np.uint32), zs[1][1].view(np.uint32))


# ---- Philox and the extreme words -----------------------------------------------------------------------------------------------------------
def test_philox_gives_the_known_answers_and_the_seeds_their_words():
    for counter, key, want in D.KNOWN_ANSWERS:
        assert tuple(int(x) for x in D.philox(counter, key)) == want, [hex(int(x)) for x in D.philox(counter, key)]
    assert set(D.EXTREME_SEEDS) == {39075, 2871038, 1343428, 56065608}
    for seed, (onehot, w, word) in D.EXTREME_SEEDS.items():
        assert int(D.words(seed, 0, 0, 0, onehot)[w]) == word, (seed, hex(int(D.words(seed, 0, 0, 0, onehot)[w])))
    u = D.u01(np.array([0xffffff7f, 0xffffffa1, 0x00000000, 0xffffff25, 0xfffffe00], np.uint32))
    assert np.all(u[[0, 1, 3]] == D.U01_MAX) and u[2] == np.float32(2.0 ** -25) and u[4] == np.float32(1.0 - 2.0 ** -23)
    assert D.u01(np.uint32(0xffffff7f), 'u01_unclamped') == np.float32(1.0)                  # 16777215.5 is no float32: it rounds to 2^24
    # the clamp moves that one value: every other top-24-bit pattern keeps its bits
    x = (np.arange(1 << 24, dtype=np.uint32) << np.uint32(8))
    a, b = D.u01(x), D.u01(x, 'u01_unclamped')
    assert np.array_equal(a[:-1].view(np.uint32), b[:-1].view(np.uint32)) and a[-1] == D.U01_MAX and b[-1] == 1.0
    # one-hot indices do not change with the clamp, for any width in use
    for K in (1, 3, 10, 30, 50, 256, 8192):
        top = np.float32(K)
        assert min(int(np.float32(1.0) * top), K - 1) == min(int(D.U01_MAX * top), K - 1) == K - 1
    assert int(D.u01(np.uint32(0xffffff25)) * np.float32(30)) == 29 and int(np.float32(1.0) * np.float32(30)) == 30
    # what the documented interval says of a = 0 and of (1, 2)
    assert np.float32(1.0) + (np.float32(2.0) - np.float32(1.0)) * D.U01_MAX == np.float32(2.0)
    for b_ in (np.float32(1.0), np.float32(1.0 / 128), np.float32(3.7)):
        assert np.float32(0) + b_ * D.U01_MAX < b_


# ---- the bounds: not too tight for the right kernel, too tight for each wrong one -----------------------------------------------------------
@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_the_float32_restatement_passes_every_bound(idx):
    row, inp = ROWS[idx], _inp(idx)
    fr, broken = D.check(row, inp, D.run32(row, inp))
    print('LATENT %s (float32 numpy) fractions of the bound: %s' % (row_id(row), ' '.join('%s %.4f' % kv for kv in sorted(fr.items()))))
    assert not broken and D.within(fr) and set(fr) <= set(D.kernels_of(row)), (fr, broken)


# the row on which each wrong kernel is shown to miss
_SIZES, _SLOTS, _WRAP = 'noise-s123456789abcdef0-c12-n1027-d5', 'noise-sc-c16-n37-d3', 'noise-sd-c3-n9-dffffffff_x'
MUTANT_ROW = {
    'philox_9_rounds': _SIZES, 'multipliers_swapped': _SIZES, 'slot_left_out': _SLOTS, 'draw_high_dropped': _WRAP, 'onehot_keyed_by_element': _SIZES,
    'u01_no_half': _SIZES, 'u01_unclamped': 'noise-s98a3-c1-n4-d0-k1-0-1', 'tail_guard_off_by_one': _SIZES, 'single_log_gumbel': 'latent-5x4x63-t0.5',
    'softmax_no_max': 'latent-5x256x130-t0.1', 'temp_multiplied': 'latent-5x5x65-t0.1', 'dlog_without_dot': 'latent-5x4x63-t0.5',
    'dz_wrong_sign': 'latent-5x4x63-t0.5', 'dmu_summed_over_K': 'latent-256x5x257-t0.5', 'last_index_wins_tie': 'latent-5x4x63-t0.5',
    'half_dropped': 'latent-5x5x65-t0.1', 'highest_row_wins_tie': 'post-k255-d65-128+3_0+3_64+3',
}


@pytest.mark.parametrize('mut', D.MUTANTS)
def test_each_wrong_kernel_misses_on_its_row(mut):
    assert set(MUTANT_ROW) == set(D.MUTANTS)
    idx = _index(MUTANT_ROW[mut])
    row, inp = ROWS[idx], _inp(idx)
    fr, broken = D.check(row, inp, D.run32(row, inp, mut))
    print('LATENT wrong kernel %s on %s: worst fraction %.3g, broken %s' % (mut, row_id(row), max(fr.values()), broken))
    assert broken or max(fr.values()) > 2.0, (fr, broken)                        # by a margin, not by a rounding
    fr, broken = D.check(row, inp, D.run32(row, inp, None))
    assert not broken and D.within(fr)


def test_the_unclamped_u01_fails_every_extreme_uniform_and_normal_row():
    """the kernel as it was before the clamp: 1.0 for the words ffffffxx"""
    for rid, what in (('noise-s98a3-c1-n4-d0-k1-0-1', 'bit for bit'), ('noise-s98a3-c1-n4-d0-k1-0-0.0078125', 'outside (0, b)'),
                      ('noise-s2bcefe-c1-n4-d0-k0-0-1', None)):
        idx = _index(rid)
        out = D.run32(ROWS[idx], _inp(idx), 'u01_unclamped')
        fr, broken = D.check(ROWS[idx], _inp(idx), out)
        assert (broken and (what is None or any(what in b for b in broken))) or not D.within(fr), (rid, fr, broken)
    idx = _index('noise-s98a3-c1-n4-d0-k1-0-1')
    assert D.run32(ROWS[idx], _inp(idx), 'u01_unclamped')['vals'][0][0][3] == 1.0 and D.run32(ROWS[idx], _inp(idx))['vals'][0][0][3] == D.U01_MAX


def test_a_nan_a_touched_pad_or_a_wrong_count_fails():
    for rid, key in (('latent-5x4x63-t0.5', 'dz'), ('latent-5x4x63-t0.5', 'k_st'), ('mix-257x100x4', 'out')):
        idx = _index(rid)
        out = D.run32(ROWS[idx], _inp(idx))
        out[key] = np.array(out[key], np.float32)
        out[key].flat[-1] = np.nan
        fr, broken = D.check(ROWS[idx], _inp(idx), out)
        assert broken and (key == 'k_st' or not D.within(fr)), (rid, fr, broken)
    idx = _index(_SIZES)
    out = D.run32(ROWS[idx], _inp(idx))
    out['vals'][0][2][-1] = np.float32(0.0)
    assert D.check(ROWS[idx], _inp(idx), out)[1]
    out = D.run32(ROWS[idx], _inp(idx))
    out['states'][0] = (ROWS[idx]['seed'], 6, 1)
    assert D.check(ROWS[idx], _inp(idx), out)[1]
    idx = _index('acc-n300-k7')
    out = D.run32(ROWS[idx], _inp(idx))
    out['correct'] += 1
    assert D.check(ROWS[idx], _inp(idx), out)[1]


def test_the_host_decode_is_evaluates(lib_built):
    from graphical_gan_amd import evaluate as E
    for idx, r in enumerate(ROWS):
        if r['entry'] == 'acc':
            i = _inp(idx)
            assert E.decode_cluster_accuracy(i['assign'], i['labels'], i['colbest']) == D.decode_accuracy(i['assign'], i['labels'], i['colbest']) > 0
        if r['entry'] == 'post':
            out = D.run32(r, _inp(idx))
            assert E.decode_cluster_accuracy(out['assign'], _inp(idx)['labels'], out['colbest']) == out['correct']
            P = np.concatenate(out['probs'])
            assert len(r['batches']) > 1 or np.array_equal(E.column_keys(P), out['colbest'])


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
    ids = [r['id'] for r in D.REJECTED]
    assert len(set(ids)) == len(ids)
    for what in ('noise-count0', 'noise-count17', 'noise-size0', 'noise-size7fffffff', 'noise-kind-1', 'noise-kind3', 'noise-width0',
                 'noise-width-does-not-divide', 'noise-null-dsts', 'noise-null-sizes', 'noise-null-kinds', 'noise-null-a', 'noise-null-b',
                 'noise-null-widths', 'noise-null-state', 'noise-null-dst', 'fwd-K257', 'bwd-K257', 'bwd-B257', 'stc_bwd-B257', 'st_bwd-B257',
                 'fwd-D0', 'bwd-D0', 'fwd-temp0', 'fwd-temp-1', 'bwd-temp0', 'bwd-temp-1', 'stc_fwd-temp0', 'stc_bwd-temp-1',
                 'bwd-both-gradients-null', 'bwd-both-outputs-null', 'stc_bwd-both-gradients-null', 'st_bwd-both-outputs-null',
                 'st_fwd-mode0', 'st_fwd-mode3', 'st_bwd-mode0', 'st_bwd-mode3', 'stc_fwd-null-u', 'stc_fwd-null-soft', 'stc_bwd-null-soft',
                 'fwd-null-z', 'fwd-null-mu', 'fwd-null-u', 'fwd-null-k', 'bwd-null-z', 'bwd-null-mu', 'bwd-null-k',
                 'mix-D6', 'mix-mu-4-bytes-off', 'mix-noise-4-bytes-off', 'mix-out-4-bytes-off', 'mix-null-k', 'post-K8193', 'post-row0-1',
                 'post-row0+B-past-2^31-1', 'post-null-assign', 'post-null-colbest', 'acc-N0', 'acc-K8193', 'acc-null-correct'):
        assert what in ids, what
