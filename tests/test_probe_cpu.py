"""not-gpu: the least-squares linear probe away from the device -- the float64 restatement tests/_probe_ref.py against np.linalg.lstsq, its
tie rule and constant columns, what the reference alone says about the GPU rows (accuracies in the middle, how few rows the margin rule
lets off), the switch and the flag, the ABI, and the argument refusals of the C entry points and of functional."""
import argparse
import ctypes as C
import glob
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_mnist', 'gan_inference_face',
                 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_mnist', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_probe_moments_workspace', 'ggan_probe_moments', 'ggan_probe_normal_workspace', 'ggan_probe_normal', 'ggan_probe_solve',
           'ggan_probe_predict']


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', range(len(R.ROWS)), ids=[R.row_id(r) for r in R.ROWS])
def test_restatement_is_the_least_squares_solution(idx):
    """the closed form equals np.linalg.lstsq on the augmented system [Zs 1; sqrt(n lambda) I 0] with an unpenalised intercept column"""
    r, x, f = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    W, b = R.lstsq_fit(x['Z'], x['y'], r['C'])
    assert np.max(np.abs(W - f['W'])) <= 1e-10 and np.max(np.abs(b - f['bias'])) <= 1e-10
    assert abs(f['bias'].sum() - 1.0) <= 1e-12 and f['counts'].sum() == r['n']
    assert np.max(np.abs(R.standardise(x['Z'], f['mean'], f['inv_std']).sum(axis=0))) <= 1e-9 * r['n']      # Zs^T 1 = 0: R needs no centring


def test_a_tie_goes_to_the_lowest_class():
    sc = np.array([[0.25, 0.5, 0.5, 0.1], [0.7, 0.7, 0.7, 0.7], [0.0, -1.0, 0.0, 0.0], [-3.0, -2.0, -2.5, -2.0]])
    assert R.predict(sc).tolist() == [1, 0, 0, 1]
    idx = [i for i, r in enumerate(R.ROWS) if 'tie' in r][0]
    (a, b), x, f = R.ROWS[idx]['tie'], R.inputs(idx), R.reference(idx)
    assert a < b and f['counts'][a] == f['counts'][b] > 0
    sc = R.scores(x['Zq'], f['mean'], f['inv_std'], f['W'], f['bias'])
    pred = R.predict(sc)
    assert not np.any(pred == b)
    assert np.allclose(sc[:, a], sc[:, b], rtol=0, atol=1e-12) and np.any(pred == a)      # (the twin would win as often, were it not for the rule)


def test_a_constant_column_drops_out():
    idx = [i for i, r in enumerate(R.ROWS) if 'const' in r][0]
    r, x, f = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    j = r['const']
    assert f['inv_std'][j] == 0 and np.all(f['inv_std'][np.arange(r['d']) != j] > 0)
    assert np.all(f['W'][j] == 0) and np.all(f['G'][j] == 0) and np.all(f['G'][:, j] == 0) and np.all(f['R'][j] == 0)
    moved = np.array(x['Zq'])
    moved[:, j] += 1e6                                   # whatever the scoring rows hold there
    same = lambda Z: R.predict(R.scores(Z, f['mean'], f['inv_std'], f['W'], f['bias']))
    assert np.array_equal(same(moved), same(x['Zq']))
    z = np.full((5, 3), 2.5, np.float32)
    mu, s, _ = R.moments(z, np.zeros(5, int), 1)
    assert np.all(s == 0) and np.all(mu == 2.5)


def test_an_absent_class_is_never_predicted():
    idx = [i for i, r in enumerate(R.ROWS) if 'absent' in r][0]
    r, x, f = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    c = r['absent']
    assert f['counts'][c] == 0 and f['bias'][c] == 0 and np.all(f['W'][:, c] == 0) and np.any(x['yq'] == c)
    assert not np.any(R.predict(R.scores(x['Zq'], f['mean'], f['inv_std'], f['W'], f['bias'])) == c)


def test_the_rows_the_gpu_tests_use():
    """on the float64 reference alone: the accuracy is in the middle on at least three rows, the margin rule lets off at most 2 % of any
    row's rows (from the reference's own float32-rounded fit), every instance of the normal-equations kernel has a row, and one row is a
    row block plus one"""
    middle = 0
    for idx, r in enumerate(R.ROWS):
        x, f = R.inputs(idx), R.reference(idx)
        f4 = lambda a: np.asarray(a, np.float32)
        for Z in (x['Z'], x['Zq']):
            _, closed, _ = R.margins(Z, f4(f['mean']), f4(f['inv_std']), f4(f['W']), f4(f['bias']), twin=r.get('tie'))
            assert 1.0 - closed.mean() <= R.OPEN_ROWS_CAP, (R.row_id(r), 1.0 - closed.mean())
        print(R.row_id(r), 'accuracy fit %.3f dev %.3f' % (f['acc_fit'], f['acc_dev']), 'float32 restatement error in W %.2e' % f['w32_err'])
        middle += R.MIDDLE[0] <= f['acc_dev'] <= R.MIDDLE[1]
        assert r['d'] <= R.MAX_DIM and r['C'] <= R.MAX_CLASSES and r['n'] >= 2
    assert middle >= 3
    assert sorted(set(R.instance(r) for r in R.ROWS)) == ['probe_normal_t%d' % t for t in (1, 2, 3, 4)]
    assert any(r['n'] == R.ROW_BLOCK + 1 for r in R.ROWS)
    assert [(r['n'], r['m'], r['d'], r['C']) for r in R.ROWS[:5]] == [(64, 40, 1, 2), (257, 131, 8, 10), (1000, 300, 37, 10), (1500, 513, 128, 13),
                                                                      (300, 100, 128, 32)]


def test_a_one_pass_variance_would_fail_on_these_inputs():
    """E[z^2] - mu^2 in float32 misses 1 / std by far more than the moments bound on the recipe's offset columns"""
    x = R.inputs(3)
    Z = x['Z']
    mu, s, _ = R.moments(Z, x['y'], 13)
    v1 = (Z * Z).mean(axis=0, dtype=np.float32) - Z.mean(axis=0, dtype=np.float32) ** 2
    s1 = 1.0 / np.sqrt(np.maximum(v1.astype(np.float64), 1e-30))
    assert np.max(np.abs(s1 - s) / s) > 1e3 * 4 * R.U


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_probe_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_PROBE_EVERY', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.probe_settings(s) == {} and run.probe_settings('/somewhere/%s.py' % s) == {}
    base = {s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s)) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_PROBE_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.probe_settings(s) == {'PROBE_EVERY': 20} and run.probe_settings('/somewhere/%s.py' % s) == {'PROBE_EVERY': 20}
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.probe_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s)) == base[s]
    S = dict(run.reference_block('gan_inference_cifar10'), **run.probe_settings('gan_inference_cifar10'))
    assert [it for it in range(60) if run.probe_due(S, it)] == [19, 39, 59]
    assert run.eval_plan(S) is None and not any(run.scores_due(S, it) for it in range(60))
    assert not any(run.probe_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_the_eight_image_scripts_carry_the_line():
    line = 'SETTINGS.update(run.probe_settings(__file__))'
    seen = {os.path.splitext(os.path.basename(p))[0]: open(p).read().count(line) for p in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py'))}
    assert seen == dict([(s, 1) for s in IMAGE_SCRIPTS] + [(s, 0) for s in SEQUENCE_SCRIPTS])


def test_probe_sets_without_labelled_training_data():
    from graphical_gan_amd import run
    state = np.random.get_state()[1].tobytes()
    assert run.probe_sets(dict(DATASET='face', BATCH_SIZE=8)) is None
    assert run.probe_sets(dict(DATASET='cifar10', BATCH_SIZE=8, SYNTHETIC='force')) is None
    assert run.probe_sets(dict(DATASET='cifar10', BATCH_SIZE=8, DATA_DIR='/no/such/dir')) is None
    assert np.random.get_state()[1].tobytes() == state


def test_the_flag_parses_and_the_state_space_scripts_refuse_it(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--probe']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert parsed[0].probe is False and parsed[1].probe is True
    assert not any(getattr(parsed[1], r.name) for r in evaluate.SET_SCORES)
    for script in SEQUENCE_SCRIPTS:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--probe', '--out-dir', 'x'])
        assert e.value.code == 2 and '--probe: the state-space scripts have no single code' in capsys.readouterr().err


def test_the_pass_is_no_row_of_the_table():
    from graphical_gan_amd import evaluate
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    sig = inspect.signature(evaluate.evaluate_once)
    names = list(sig.parameters)
    assert names.index('probe') < names.index('scores') and sig.parameters['probe'].default is False
    assert sig.parameters['scores'].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError, match='no set-level score probe'):
        evaluate._known('set_scores', dict(probe=True))
    assert evaluate.PROBE_KEYS == ('dev probe accuracy z', 'fit probe accuracy z', 'dev probe accuracy xr')
    assert (evaluate.PROBE_FIT_ROWS, evaluate.PROBE_MAX_ROWS, evaluate.PROBE_RIDGE) == (10000, 10000, 1e-2)
    ev = object.__new__(evaluate.Evaluator)
    ev.S = {}
    xs = [(np.zeros((4, 6), np.float32), np.zeros(4, np.int64))]
    with pytest.raises(ValueError, match='labelled'):
        ev.probe_scores(xs, [np.zeros((4, 6), np.float32)])
    with pytest.raises(ValueError, match='labelled'):
        ev.probe_scores([], xs)
    ev.S = dict(PROBE_RIDGE=0.0)
    with pytest.raises(ValueError, match='PROBE_RIDGE'):
        ev.probe_scores(xs, xs)
    ev.S = {}
    with pytest.raises(ValueError, match='at most 32 classes'):
        ev.probe_scores(xs, [(xs[0][0], np.full(4, 32))])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_800_and_the_entry_points_are_bound(lib_built):
    from graphical_gan_amd import _lib, build, functional as F
    lib = _lib.load()
    assert lib.ggan_version() == _lib.ABI_VERSION == 800
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert '#define GGAN_ABI_VERSION 800' in hdr and 'probe_fit.hip' in build.SOURCES
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    const = lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
    assert (F.PROBE_MAX_DIM, F.PROBE_MAX_CLASSES, F.PROBE_ROW_BLOCK) == (const('GGAN_PROBE_MAX_DIM'), const('GGAN_PROBE_MAX_CLASSES'),
                                                                        const('GGAN_PROBE_ROW_BLOCK')) == (R.MAX_DIM, R.MAX_CLASSES, R.ROW_BLOCK)
    assert (F.PROBE_BAD_LABEL, F.PROBE_NONFINITE, F.PROBE_BAD_PIVOT) == (const('GGAN_PROBE_BAD_LABEL'), const('GGAN_PROBE_NONFINITE'),
                                                                         const('GGAN_PROBE_BAD_PIVOT')) == (R.BAD_LABEL, R.NONFINITE, R.BAD_PIVOT)


def test_the_entry_points_refuse_bad_arguments_before_any_launch(lib_built):
    """null pointers, shapes beyond the caps, n < 2, a ridge that is not positive, a short or misaligned workspace: a negative code and a
    message, on a machine with no device to launch on"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    p, big = C.c_void_p(4096), 1 << 30

    def refused(rc, what):
        assert rc < 0 and what.encode() in L.ggan_last_error(), (rc, what, L.ggan_last_error())
    assert L.ggan_probe_moments_workspace(100, 8, 10) > 0 and L.ggan_probe_normal_workspace(100, 8, 10) >= 4 * (64 + 80)
    for bad in ((1, 8, 10), (100, 0, 10), (100, 129, 10), (100, 8, 0), (100, 8, 33), (131073, 8, 10)):
        assert L.ggan_probe_moments_workspace(*bad) == 0 and L.ggan_probe_normal_workspace(*bad) == 0, bad
    mom = lambda n=100, d=8, c=10, Z=p, ws=p, nb=big: L.ggan_probe_moments(Z, p, n, d, c, p, p, p, p, ws, nb, None)
    nor = lambda n=100, d=8, c=10, G=p, ws=p, nb=big: L.ggan_probe_normal(p, p, n, d, c, p, p, G, p, ws, nb, None)
    sol = lambda n=100, d=8, c=10, ridge=0.01, W=p: L.ggan_probe_solve(p, p, p, n, d, c, ridge, W, p, p, None)
    pre = lambda m=100, d=8, c=10, y=p, pred=p, correct=p: L.ggan_probe_predict(p, y, m, d, c, p, p, p, p, pred, correct, None)
    for fn in (mom, nor, sol):
        refused(fn(d=129), 'd <= 128')
        refused(fn(d=0), 'd <= 128')
        refused(fn(c=33), 'classes <= 32')
        refused(fn(n=1), 'n < 2')
        refused(fn(n=131073), '131072')
    refused(mom(Z=None), 'null pointer')
    refused(nor(G=None), 'null pointer')
    refused(sol(W=None), 'null pointer')
    for fn in (mom, nor):
        refused(fn(nb=16), 'workspace too small')
        refused(fn(ws=C.c_void_p(4100)), '16-byte aligned')
    for ridge in (0.0, -1.0, float('nan'), float('inf')):
        refused(sol(ridge=ridge), 'ridge')
    refused(pre(d=129), 'd <= 128')
    refused(pre(c=0), 'classes <= 32')
    refused(pre(m=0), '1 <= m')
    refused(pre(pred=None, correct=None), 'nothing to write')
    refused(pre(y=None), 'correct needs the labels')


def test_functional_refuses_what_it_must_before_the_device():
    import torch
    from graphical_gan_amd import functional as F, _lib
    z, y = torch.zeros(10, 4), torch.zeros(10, dtype=torch.int32)
    for kw, what in ((dict(z=torch.zeros(10, 129)), 'columns'), (dict(classes=33), 'classes'), (dict(classes=0), 'classes'),
                     (dict(z=torch.zeros(1, 4), y=y[:1]), 'at least 2 rows'), (dict(ridge=0.0), 'ridge'), (dict(ridge=-1.0), 'ridge'),
                     (dict(ridge=float('nan')), 'ridge'), (dict(z=z.double()), 'float32'), (dict(y=y.long()), 'int32'), (dict(y=y[:9]), 'int32'),
                     (dict(z=torch.zeros(10)), 'float32 rows')):
        a = dict(dict(z=z, y=y, classes=3, ridge=0.01), **kw)
        with pytest.raises(ValueError, match=what):
            F.lsq_probe_fit(a['z'], a['y'], a['classes'], a['ridge'])
    with pytest.raises(_lib.GganError, match='no backward'):
        F.lsq_probe_fit(z.clone().requires_grad_(), y, 3, 0.01)
    with pytest.raises(_lib.GganError, match='no CPU path'):           # no fall-back
        F.lsq_probe_fit(z, y, 3, 0.01)
    new = lambda *s: torch.zeros(*s)
    fit = F.ProbeFit(new(4), new(4), new(4, 3), new(3), torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='4 columns'):
        F.lsq_probe_predict(fit, torch.zeros(10, 5))
    with pytest.raises(ValueError, match='int32'):
        F.lsq_probe_predict(fit, z, y.long())
    with pytest.raises(_lib.GganError, match='no CPU path'):
        F.lsq_probe_predict(fit, z, y)
