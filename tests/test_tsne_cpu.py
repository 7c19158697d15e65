"""The host side of the latent-space t-SNE pass: the ABI of csrc/tsne.hip and its argument checks, the float64 restatement
tests/_tsne_ref.py pinned to scikit-learn's results (tests/golden/tsne_reference.json, written by tests/golden/make_tsne_fixture.py),
tflib.visualization.scatter, and the pass's cadence."""
import ctypes as C
import json
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tsne_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TSNE_SYMBOLS = ('ggan_tsne_sqnorms', 'ggan_tsne_neighbours', 'ggan_tsne_affinities', 'ggan_tsne_symmetrise', 'ggan_tsne_gradient',
                'ggan_tsne_kl', 'ggan_tsne_iterate')


@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(GOLDEN, 'tsne_reference.json')) as f:
        fx = json.load(f)
    fx['bh'] = np.load(os.path.join(GOLDEN, 'tsne_reference_bh.npy'))
    fx['X'], fx['y'] = R.fixture_inputs(fx['recipe'])
    fx['P'] = R.sparse_P(fx['X'], fx['perplexity'])
    return fx


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from graphical_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert int(re.search(r'#define GGAN_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == 800        # additive: no new version
    assert int(re.search(r'#define GGAN_TSNE_MAX_K (\d+)', hdr).group(1)) == _lib.TSNE_MAX_K == 128
    assert int(re.search(r'#define GGAN_TSNE_MAX_SPLITS (\d+)', hdr).group(1)) == _lib.TSNE_MAX_SPLITS == 64
    L = _lib.load()
    for name in TSNE_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(r'\bint %s\(' % name, hdr), name
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, hdr).group(1)
        assert len(getattr(L, name).argtypes) == decl.count(',') + 1, name
    assert 'tsne.hip' in __import__('graphical_gan_amd.build', fromlist=['SOURCES']).SOURCES


def test_argument_checks_answer_without_a_gpu():
    from graphical_gan_amd import _lib
    L = _lib.load()
    p, n = C.c_void_p(16), C.c_void_p(0)
    err = lambda: L.ggan_last_error().decode()
    assert L.ggan_tsne_sqnorms(n, 10, 4, p, n) != 0 and 'null' in err()
    assert L.ggan_tsne_sqnorms(p, 0, 4, p, n) != 0
    nb = L.ggan_tsne_neighbours
    assert nb(p, p, 100, 4, 0, 100, 10, n, p, p, n, 0, n) != 0 and 'null' in err()
    assert nb(p, p, 1000, 4, 0, 100, 129, p, p, p, n, 0, n) != 0 and 'K' in err()                   # K <= 128
    assert nb(p, p, 1, 4, 0, 1, 1, p, p, p, n, 0, n) != 0 and 'N' in err()                          # N >= 2
    assert nb(p, p, 10, 4, 0, 10, 10, p, p, p, n, 0, n) != 0                                        # K < N: self is excluded
    assert nb(p, p, 100, 4, 60, 50, 10, p, p, p, n, 0, n) != 0 and 'block' in err()                 # rows beyond the data
    af = L.ggan_tsne_affinities
    assert af(p, 100, 90, 30.0, 100, 1e-5, n, p, n) != 0 and 'null' in err()
    assert af(p, 100, 90, 100.0, 100, 1e-5, p, p, n) != 0 and 'perplexity' in err()                 # perplexity >= N
    assert af(p, 100, 90, 0.0, 100, 1e-5, p, p, n) != 0
    assert af(p, 1, 1, 0.5, 100, 1e-5, p, p, n) != 0                                                # N >= 2
    assert af(p, 1000, 129, 30.0, 100, 1e-5, p, p, n) != 0                                          # K <= 128
    assert af(p, 1000, 90, 30.0, 0, 1e-5, p, p, n) != 0                                             # the search is bounded by count
    sy = L.ggan_tsne_symmetrise
    assert sy(p, p, 100, 10, p, p, p, n, n) != 0 and 'null' in err()
    assert sy(p, p, 1, 1, p, p, p, p, n) != 0 and sy(p, p, 1000, 129, p, p, p, p, n) != 0
    gr = L.ggan_tsne_gradient
    assert gr(p, p, p, n, 100, 4, p, p, p, p, p, n) != 0 and 'null' in err()
    assert gr(p, p, p, p, 1, 4, p, p, p, p, p, n) != 0 and 'N' in err()
    assert gr(p, p, p, p, 100, 0, p, p, p, p, p, n) != 0 and 'splits' in err()
    assert gr(p, p, p, p, 100, 65, p, p, p, p, p, n) != 0 and 'splits' in err()
    assert gr(p, p, p, p, 100, 4, p, p, n, p, p, n) != 0
    assert L.ggan_tsne_kl(p, p, p, p, 100, 4, p, p, n, p, n) != 0
    it = L.ggan_tsne_iterate
    assert it(p, p, p, p, n, p, p, 100, 4, p, p, 0, 1, 250, 12.0, 0.5, 0.8, 200.0, 0.01, n) != 0
    assert it(p, p, p, p, p, p, p, 100, 4, p, p, 0, 1, 250, 12.0, 0.5, 0.8, 200.0, 0.01, n) != 0 and 'aliased' in err()   # ya is yb
    assert it(p, p, p, p, C.c_void_p(32), p, p, 100, 4, p, p, 5, 4, 250, 12.0, 0.5, 0.8, 200.0, 0.01, n) != 0 and 'iteration' in err()


def test_product_functions_refuse_cpu_tensors():
    import torch
    from graphical_gan_amd import _lib
    from graphical_gan_amd import functional as F
    with pytest.raises(_lib.GganError):
        F.tsne(torch.zeros(100, 4))
    with pytest.raises(_lib.GganError):
        F.tsne_neighbours(torch.zeros(100, 4), 10)
    assert F.tsne_splits(10000) == 26 and F.tsne_splits(1200) == 64 and F.tsne_splits(10 ** 6) == 1


# ---- the restatement, pinned to the reference ----------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_measured(fixture):
    runs = fixture['runs']
    assert sorted((r['method'], r['seed']) for r in runs) == [(m, s) for m in ('barnes_hut', 'exact') for s in (0, 1, 2)]
    assert all(r['n_iter_'] == 999 and r['purity'] == 1.0 for r in runs)          # the reference never stops early on these inputs
    assert fixture['X'].shape == (1200, 32) and fixture['X'].dtype == np.float32 and fixture['bh'].shape == (3, 1200, 2)


def test_kl_s_of_the_recorded_reference_embeddings(fixture):
    for r in fixture['runs']:
        if r['method'] == 'barnes_hut':
            got = R.kl_sparse(fixture['P'], fixture['bh'][r['seed']])
            print('barnes_hut seed %d: KL_s %.6f recorded %.6f (sklearn reports %.6f)' % (r['seed'], got, r['kl_s'], r['kl_divergence_']))
            assert abs(got - r['kl_s']) <= 1e-9 * abs(r['kl_s'])


def test_restatement_replays_its_recorded_prefix(fixture):
    """the first 10 iterations from each seed's start: the recorded positions, within 1e-6 of the embedding's extent.  (The prefix stops
    at 10: a change of 1e-16 in P grows to 1e-15 of the extent by iteration 10 and to 1e-6 by iteration 50, where the comparison would
    depend on the machine's summation order.)"""
    its, npts = fixture['prefix_iters'], fixture['prefix_points']
    for rec in fixture['restatement']:
        _, kept = R.run(fixture['P'], R.initial(len(fixture['X']), rec['seed']), max(its), keep=its)
        for it in its:
            want, extent = np.asarray(rec['prefix'][str(it)]), rec['extent'][str(it)]
            err = np.abs(kept[it][:npts] - want).max() / extent
            print('seed %d iteration %d: %.3g of the extent %.4g' % (rec['seed'], it, err, extent))
            assert err <= 1e-6


def test_restatement_is_no_worse_than_barnes_hut(fixture):
    lowest_bh = min(r['kl_s'] for r in fixture['runs'] if r['method'] == 'barnes_hut')
    for rec in fixture['restatement']:
        assert rec['kl_s'] <= lowest_bh and rec['purity'] == 1.0, rec['seed']


def test_near_ties_at_the_neighbour_boundary_are_rare(fixture):
    """the condition on the inputs that keeps the GPU neighbour test meaningful: at most 1 % of rows may have neighbours 90 and 91
    closer than the fp32 rounding of a GEMM-form distance, 4 * 2^-23 * (|x_i|^2 + max_j |x_j|^2)"""
    X = fixture['X'].astype(np.float64)
    s = np.sort(R.sq_distances(X), axis=1)
    nrm = (X ** 2).sum(1)
    near = int(((s[:, 90] - s[:, 89]) < 4 * 2.0 ** -23 * (nrm + nrm.max())).sum())
    print('rows with a near-tie at the boundary: %d of %d' % (near, len(X)))
    assert near <= 0.01 * len(X)


# ---- tflib.visualization -------------------------------------------------------------------------------------------------------------
def read_png(path):
    """8-bit RGB / grey PNG as save_images.write_png writes it (filter 0 on every line) -> uint8 array"""
    b = open(path, 'rb').read()
    assert b[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(b):
        n, tag = struct.unpack('>I', b[pos:pos + 4])[0], b[pos + 4:pos + 8]
        data = b[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', b[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', data)
        elif tag == b'IDAT':
            idat += data
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    ch = {0: 1, 2: 3}[ctype]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert depth == 8 and not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, ch)


def test_scatter_files_colours_and_placement(tmp_path):
    before = set(sys.modules)
    from graphical_gan_amd import tflib as lib
    V = lib.visualization
    rng = np.random.RandomState(3)
    # two classes: 0 on the left, 1 on the right
    data = np.concatenate([rng.normal(size=(200, 2)) * 0.3 + [-3, 0], rng.normal(size=(200, 2)) * 0.3 + [3, 0]])
    label = np.repeat([0, 1], 200)
    d = str(tmp_path)
    V.scatter(data, label, d, 'toy.png', mus=np.array([[-3., 0.], [3., 0.]]))
    assert sorted(os.listdir(d)) == ['mus_toy.png', 'toy.png']
    img = read_png(os.path.join(d, 'toy.png'))
    assert img.shape == (V.SIZE, V.SIZE, 3)
    c0, c1 = (np.all(img == np.asarray(V.PALETTE[k], np.uint8), axis=2) for k in (0, 1))
    half = V.SIZE // 2
    assert c0[:, :half].sum() > 100 and c0[:, half:].sum() == 0 and c1[:, half:].sum() > 100 and c1[:, :half].sum() == 0
    mus = read_png(os.path.join(d, 'mus_toy.png'))
    m0 = np.all(mus == np.asarray(V.PALETTE[0], np.uint8), axis=2)
    assert m0.sum() > 4 * 9 and m0[:, half:].sum() == 0                  # larger marks than the data's
    # one-hot labels are the integer labels, byte for byte
    V.scatter(data, np.eye(2)[label], d, 'onehot.png')
    assert open(os.path.join(d, 'onehot.png'), 'rb').read() == open(os.path.join(d, 'toy.png'), 'rb').read()
    # every class colour is present: 10 classes from the palette, 30 from the hue wheel, all distinct
    for n in (10, 30):
        pts = rng.uniform(-1, 1, size=(n * 20, 2))
        lab = np.tile(np.arange(n), 20)
        V.scatter(pts, lab, d, 'many%d.png' % n)
        img = read_png(os.path.join(d, 'many%d.png' % n)).reshape(-1, 3)
        cols = V.class_colours(n)
        assert len({tuple(c) for c in cols}) == n
        seen = {tuple(c) for c in np.unique(img, axis=0)}
        assert all(tuple(c) in seen for c in cols), n
    # y grows upwards
    V.scatter(np.array([[0., 0.], [0., 1.]]), np.array([0, 1]), d, 'up.png', mark_size=20)
    up = read_png(os.path.join(d, 'up.png'))
    rows1 = np.where(np.all(up == np.asarray(V.PALETTE[1], np.uint8), axis=2))[0]
    rows0 = np.where(np.all(up == np.asarray(V.PALETTE[0], np.uint8), axis=2))[0]
    assert rows1.mean() < rows0.mean()
    assert not {m.split('.')[0] for m in set(sys.modules) - before} & {'seaborn', 'pandas', 'matplotlib', 'PIL'}


# ---- cadence -------------------------------------------------------------------------------------------------------------------------
def test_manifold_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_MANIFOLD_EVERY', raising=False)
    scripts = sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, 'scripts')) if f.endswith('.py'))
    assert len(scripts) == 10
    before = {s: run.eval_settings(s) for s in scripts}
    for s in scripts:
        want = {'gan_inference_mnist': {'MANIFOLD_EVERY': 50000}, 'gmgan_inference_mnist': {'MANIFOLD_AT_END': True}}.get(s, {})
        assert run.manifold_settings(s) == want and run.manifold_settings('/somewhere/%s.py' % s) == want
        src = open(os.path.join(ROOT, 'scripts', s + '.py')).read()
        assert ('SETTINGS.update(run.manifold_settings(__file__))' in src) == bool(want), s
        assert not set(run.MANIFOLD_KEYS) & set(run.reference_block(s)) and not set(run.MANIFOLD_KEYS) & set(run.EVAL_KEYS)
    monkeypatch.setenv('GGAN_MANIFOLD_EVERY', '20')
    assert run.manifold_settings('gan_inference_mnist') == {'MANIFOLD_EVERY': 20}
    assert run.manifold_settings('gmgan_inference_mnist') == {'MANIFOLD_AT_END': True, 'MANIFOLD_EVERY': 20}
    assert run.manifold_settings('gan_inference_cifar10') == {}
    assert {s: run.eval_settings(s) for s in scripts} == before                # the other passes' settings do not know the switch
    monkeypatch.delenv('GGAN_MANIFOLD_EVERY')
    iters = 200000
    plan = run.manifold_plan(dict(run.reference_block('gan_inference_mnist'), **run.manifold_settings('gan_inference_mnist')))
    assert [it for it in range(iters) if run.manifold_due(plan, it, iters)] == [49999, 99999, 149999, 199999]
    plan = run.manifold_plan(dict(run.reference_block('gmgan_inference_mnist'), **run.manifold_settings('gmgan_inference_mnist')))
    assert [it for it in range(iters) if run.manifold_due(plan, it, iters)] == [iters - 1]
    assert run.manifold_plan(run.reference_block('gan_inference_cifar10')) is None and not run.manifold_due(None, 49999, iters)
    assert run.eval_plan(dict(run.reference_block('gmgan_inference_mnist'), **run.manifold_settings('gmgan_inference_mnist'))) is None
    assert run.labelled([(np.zeros(3), np.zeros(3))]) and not run.labelled([np.zeros(3)]) and not run.labelled([])


def test_cli_refuses_manifold_before_building_anything(tmp_path, capsys):
    """--manifold for a script that has no such pass, or without --out-dir: refused with the real reason, before the checkpoint (which
    does not even exist here) is opened"""
    from graphical_gan_amd import evaluate
    ckpt = str(tmp_path / 'missing.npz')
    for script in ('gan_inference_cifar10', 'ssgan_inference_chairs'):
        with pytest.raises(SystemExit):
            evaluate.main([ckpt, '--script', script, '--out-dir', str(tmp_path), '--manifold'])
        assert 'exist for gan_inference_mnist and gmgan_inference_mnist only' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate.main([ckpt, '--script', 'gmgan_inference_mnist', '--manifold'])
    assert 'needs --out-dir' in capsys.readouterr().err
