"""not-gpu: the wide least-squares probe away from the device -- the header's constants against functional's and the tests' launch plan,
the argument refusals of the C entry points and of functional, the switch, the flag and the key tuple, and what the float64 reference alone
says about the rows the GPU tests use (how few rows the margin rule lets off)."""
import argparse
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_ref as P  # noqa: E402
import _wprobe_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_mnist', 'gan_inference_face',
                 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_mnist', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_wprobe_moments_workspace', 'ggan_wprobe_moments', 'ggan_wprobe_normal', 'ggan_wprobe_factor', 'ggan_wprobe_solve',
           'ggan_wprobe_predict']


def _header():
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    return hdr, lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_and_the_constants_agree(lib_built):
    from graphical_gan_amd import _lib, build, functional as F
    lib = _lib.load()
    hdr, const = _header()
    assert 'probe_wide.hip' in build.SOURCES and lib.ggan_version() == _lib.ABI_VERSION == const('GGAN_ABI_VERSION')      # (no version change)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    head = (const('GGAN_WPROBE_MAX_DIM'), const('GGAN_WPROBE_TILE'), const('GGAN_WPROBE_PANEL'), const('GGAN_WPROBE_CHUNK'))
    assert (F.WPROBE_MAX_DIM, F.WPROBE_TILE, F.WPROBE_PANEL, F.WPROBE_CHUNK) == head == (R.MAX_DIM, R.TILE, R.NB, R.CHUNK)
    assert head[0] == 4096 and const('GGAN_PROBE_MAX_DIM') == P.MAX_DIM == 128      # the narrow chain keeps its cap


def test_the_launch_plan_follows_the_header():
    """_wprobe_ref.launches is written in the header's tile edge, panel step and chunk: the labels carry them, the grids follow from them"""
    _, const = _header()
    T, NB, CH, B = const('GGAN_WPROBE_TILE'), const('GGAN_WPROBE_PANEL'), const('GGAN_WPROBE_CHUNK'), const('GGAN_PROBE_ROW_BLOCK')
    r = dict(n=1300, m=200, d=8 * NB + 8, C=32)
    got = R.launches(r)
    nt = -(-r['d'] // T)
    assert got[('wprobe_normal_t%d' % T, (nt * (nt + 1) // 2 + nt) * 256)] == 1
    assert sum(v for (k, _), v in got.items() if k == 'wprobe_chol_diag_nb%d' % NB) == -(-r['d'] // NB) == 9
    assert sum(v for (k, _), v in got.items() if k == 'wprobe_chol_trail_nb%d' % NB) == (r['d'] - 1) // NB == 8
    assert got[('wprobe_chol_trail_nb%d' % NB, 36 * 256)] == 1 and got[('wprobe_chol_trail_nb%d' % NB, 256)] == 1      # 8 x 8 tiles first, one last
    assert got[('wprobe_chol_panel_nb%d' % NB, NB)] == 1                    # the 8 rows under the last full block
    assert got[('wprobe_colsum', -(-r['n'] // B) * -(-r['d'] // 256) * 256)] == 1 and got[('wprobe_solve_nb%d' % NB, r['C'] * 256)] == 1
    assert got[('wprobe_predict_c%d' % CH, -(-r['n'] // 64) * 256)] == 1
    one = R.launches(dict(n=64, m=64, d=NB, C=2))                           # one panel: no panel solve, no trailing update; n = m: one key, twice
    assert not [k for k in one if 'panel' in k[0] or 'trail' in k[0]] and one[('wprobe_predict_c%d' % CH, 256)] == 2
    assert [(r['n'], r['d'], r['C']) for r in R.ROWS] == [(300, 129, 10), (512, 4 * NB, 32), (150, 200, 3), (1300, 8 * NB + 8, 32), (700, 96, 10)]


def test_the_entry_points_refuse_bad_arguments_before_any_launch(lib_built):
    """null pointers, shapes beyond the caps, n < 2, a ridge that is not positive, a short or misaligned workspace, a misaligned fp64
    matrix: a negative code and a message, on a machine with no device to launch on"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    p, big = C.c_void_p(4096), 1 << 30

    def refused(rc, what):
        assert rc < 0 and what.encode() in L.ggan_last_error(), (rc, what, L.ggan_last_error())
    assert L.ggan_wprobe_moments_workspace(100, 129, 10) >= 8 * 129 * 2 and L.ggan_wprobe_moments_workspace(131072, 4096, 32) > 0
    for bad in ((1, 8, 10), (100, 0, 10), (100, 4097, 10), (100, 8, 0), (100, 8, 33), (131073, 8, 10), (-5, 8, 10)):
        assert L.ggan_wprobe_moments_workspace(*bad) == 0, bad
    mom = lambda n=100, d=200, c=10, Z=p, ws=p, nb=big: L.ggan_wprobe_moments(Z, p, n, d, c, p, p, p, p, ws, nb, None)
    nor = lambda n=100, d=200, c=10, G=p, R_=p: L.ggan_wprobe_normal(p, p, n, d, c, p, p, G, R_, None)
    fac = lambda d=200, ridge=0.01, G=p, st=p: L.ggan_wprobe_factor(G, d, ridge, st, None)
    sol = lambda n=100, d=200, c=10, Lm=p, W=p: L.ggan_wprobe_solve(Lm, p, p, n, d, c, W, p, p, None)
    pre = lambda m=100, d=200, c=10, y=p, pred=p, correct=p: L.ggan_wprobe_predict(p, y, m, d, c, p, p, p, p, pred, correct, None)
    for fn in (mom, nor, sol):
        refused(fn(d=4097), 'd <= 4096')
        refused(fn(d=0), 'd <= 4096')
        refused(fn(c=33), 'classes <= 32')
        refused(fn(c=0), 'classes <= 32')
        refused(fn(n=1), 'n < 2')
        refused(fn(n=131073), '131072')
    refused(mom(Z=None), 'null pointer')
    refused(mom(ws=None), 'null pointer')
    refused(nor(G=None), 'null pointer')
    refused(sol(W=None), 'null pointer')
    refused(fac(G=None), 'null pointer')
    refused(fac(st=None), 'null pointer')
    refused(mom(nb=16), 'workspace too small')
    refused(mom(ws=C.c_void_p(4100)), '16-byte aligned')
    refused(nor(G=C.c_void_p(4100)), '8-byte aligned')
    refused(nor(R_=C.c_void_p(4100)), '8-byte aligned')
    refused(fac(G=C.c_void_p(4100)), '8-byte aligned')
    refused(sol(Lm=C.c_void_p(4100)), '8-byte aligned')
    refused(fac(d=0), 'd <= 4096')
    refused(fac(d=4097), 'd <= 4096')
    for ridge in (0.0, -1.0, float('nan'), float('inf')):
        refused(fac(ridge=ridge), 'ridge')
    refused(pre(d=4097), 'd <= 4096')
    refused(pre(c=0), 'classes <= 32')
    refused(pre(m=0), '1 <= m')
    refused(pre(pred=None, correct=None), 'nothing to write')
    refused(pre(y=None), 'correct needs the labels')


def test_functional_refuses_what_it_must_before_the_device():
    import torch
    from graphical_gan_amd import functional as F, _lib
    z, y = torch.zeros(10, 200), torch.zeros(10, dtype=torch.int32)
    for kw, what in ((dict(z=torch.zeros(10, 4097)), 'columns'), (dict(classes=33), 'classes'), (dict(classes=0), 'classes'),
                     (dict(z=torch.zeros(1, 200), y=y[:1]), 'at least 2 rows'), (dict(ridge=0.0), 'ridge'), (dict(ridge=float('nan')), 'ridge'),
                     (dict(z=z.double()), 'float32'), (dict(y=y.long()), 'int32'), (dict(y=y[:9]), 'int32'), (dict(z=torch.zeros(10)), 'float32 rows')):
        a = dict(dict(z=z, y=y, classes=3, ridge=0.01), **kw)
        with pytest.raises(ValueError, match=what):
            F.lsq_probe_fit_wide(a['z'], a['y'], a['classes'], a['ridge'])
    with pytest.raises(_lib.GganError, match='no backward'):
        F.lsq_probe_fit_wide(z.clone().requires_grad_(), y, 3, 0.01)
    with pytest.raises(_lib.GganError, match='no CPU path'):           # no fall-back
        F.lsq_probe_fit_wide(z, y, 3, 0.01)
    with pytest.raises(ValueError, match='columns'):                   # the narrow pair keeps its cap
        F.lsq_probe_fit(z, y, 3, 0.01)
    new = lambda *s: torch.zeros(*s)
    fit = F.ProbeFit(new(200), new(200), new(200, 3), new(3), torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='200 columns'):
        F.lsq_probe_predict_wide(fit, torch.zeros(10, 201))
    with pytest.raises(ValueError, match='int32'):
        F.lsq_probe_predict_wide(fit, z, y.long())
    with pytest.raises(_lib.GganError, match='no CPU path'):
        F.lsq_probe_predict_wide(fit, z, y)
    assert F.WPROBE_MAX_DIM == 4096


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_probe_settings_with_and_without_the_wide_switch(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_PROBE_EVERY', raising=False)
    monkeypatch.delenv('GGAN_PROBE_WIDE', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.probe_settings(s) == {}
    monkeypatch.setenv('GGAN_PROBE_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.probe_settings(s) == {'PROBE_EVERY': 20}              # unset: today's dict
    base = {s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s)) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_PROBE_WIDE', '1')
    for s in IMAGE_SCRIPTS:
        assert run.probe_settings(s) == {'PROBE_EVERY': 20, 'PROBE_WIDE': True} == run.probe_settings('/somewhere/%s.py' % s)
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.probe_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s)) == base[s]
    monkeypatch.setenv('GGAN_PROBE_WIDE', '0')
    assert run.probe_settings(IMAGE_SCRIPTS[0]) == {'PROBE_EVERY': 20}
    monkeypatch.setenv('GGAN_PROBE_WIDE', '1')
    monkeypatch.delenv('GGAN_PROBE_EVERY')
    assert run.probe_settings(IMAGE_SCRIPTS[0]) == {'PROBE_WIDE': True}
    assert not any(run.probe_due(dict(run.reference_block(IMAGE_SCRIPTS[0]), **run.probe_settings(IMAGE_SCRIPTS[0])), it) for it in range(60))


def test_the_keys_the_flag_and_the_keywords(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    from graphical_gan_amd.models import GraphicalGAN
    assert evaluate.PROBE_WIDE_KEYS == ('dev probe accuracy x', 'fit probe accuracy x', 'dev probe accuracy h', 'fit probe accuracy h')
    assert evaluate.PROBE_KEYS == ('dev probe accuracy z', 'fit probe accuracy z', 'dev probe accuracy xr')
    sig = inspect.signature(evaluate.evaluate_once).parameters
    assert sig['probe_wide'].default is False and sig['probe'].default is False
    assert inspect.signature(evaluate.Evaluator.probe_scores).parameters['wide'].default is False
    assert inspect.signature(GraphicalGAN.Extractor).parameters['return_top'].default is False
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--probe'], ['--probe-wide']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert [(a.probe, a.probe_wide) for a in parsed] == [(False, False), (True, False), (False, True)]
    for script in SEQUENCE_SCRIPTS:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--probe-wide', '--out-dir', 'x'])
        assert e.value.code == 2 and '--probe: the state-space scripts have no single code' in capsys.readouterr().err
    ev = object.__new__(evaluate.Evaluator)
    ev.S = dict(PROBE_WIDE=True, PROBE_WIDE_RIDGE=0.0)
    xs = [(np.zeros((4, 6), np.float32), np.zeros(4, np.int64))]
    with pytest.raises(ValueError, match='PROBE_WIDE_RIDGE'):
        ev.probe_scores(xs, xs)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_are_fit_for_the_gpu_before_it_sees_them():
    """on the float64 reference alone (its fit rounded to float32, as the device stores it): the margin rule lets off at most HALF of
    OPEN_ROWS_CAP of any row's rows; the special row is what its comment says; one width is the first the narrow chain refuses"""
    _, const = _header()
    cap, block = const('GGAN_WPROBE_MAX_DIM'), const('GGAN_PROBE_ROW_BLOCK')
    assert block == P.ROW_BLOCK and any(r['n'] > block and r['n'] % block for r in R.ROWS) and any(r['n'] % block == 0 for r in R.ROWS)
    for idx, r in enumerate(R.ROWS):
        x, f = R.inputs(idx), R.reference(idx)
        f4 = lambda a: np.asarray(a, np.float32)
        assert 2 <= r['n'] and 1 <= r['d'] <= cap and 1 <= r['C'] <= P.MAX_CLASSES
        for Z in (x['Z'], x['Zq']):
            W = f4(f['W'])
            if 'tie' in r:
                W[:, r['tie'][1]] = W[:, r['tie'][0]]        # (what the device guarantees bit for bit; float64 numpy only to rounding)
            _, closed, _, _ = R.margins(Z, f4(f['mean']), f4(f['inv_std']), W, f4(f['bias']), twin=r.get('tie'))
            print(R.row_id(r), 'open rows %.4f' % (1.0 - closed.mean()), 'float32 restatement error in W %.2e' % f['w32_err'])
            assert 1.0 - closed.mean() <= 0.5 * P.OPEN_ROWS_CAP, (R.row_id(r), 1.0 - closed.mean())
    assert R.ROWS[0]['d'] == P.MAX_DIM + 1 and R.ROWS[4]['d'] <= P.MAX_DIM
    r, x, f = R.ROWS[2], R.inputs(2), R.reference(2)
    (a, b), c, j = r['tie'], r['absent'], r['const']
    assert r['n'] < r['d'] and np.linalg.matrix_rank(f['G']) < r['d'] and np.all(np.linalg.eigvalsh(f['G'] + float(P.RIDGE) * np.eye(r['d'])) > 0)
    assert f['counts'][a] == f['counts'][b] == r['n'] // 2 and f['counts'][c] == 0 and np.any(x['yq'] == c)
    assert f['inv_std'][j] == 0 and np.all(f['G'][j] == 0) and np.all(f['W'][j] == 0) and np.all(f['W'][:, c] == 0)
    assert np.array_equal(x['Z'][0::2], x['Z'][1::2])


def test_a_one_pass_variance_would_fail_on_these_inputs():
    from graphical_gan_amd import functional as F
    assert R.ROWS[0]['d'] <= F.WPROBE_MAX_DIM                      # (a row of the wide chain)
    x = R.inputs(0)
    Z = x['Z']
    mu, s, _ = P.moments(Z, x['y'], R.ROWS[0]['C'])
    v1 = (Z * Z).mean(axis=0, dtype=np.float32) - Z.mean(axis=0, dtype=np.float32) ** 2
    s1 = 1.0 / np.sqrt(np.maximum(v1.astype(np.float64), 1e-30))
    assert np.max(np.abs(s1 - s) / s) > 10 * 4 * P.U
