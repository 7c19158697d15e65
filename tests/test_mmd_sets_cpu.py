"""not-gpu: the set-level MMD op's ABI (header, binding, built library, argument errors without a GPU), the cadence settings of the
dev-set MMD pass and of the five set-level scores together, their table, the scripts' one line for them, and the float64 restatement tests/_mmd_ref.py against the oracle and the reference's formula."""
import argparse
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mmd_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_mix_rbf_sums_workspace', 'ggan_mix_rbf_sums', 'ggan_mix_rbf_mmd2_unbiased_fwd', 'ggan_mix_rbf_mmd2_unbiased_bwd')
IMAGE_SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')]
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']


def test_header_binding_and_library_agree(lib_built):
    from graphical_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = C.CDLL(lib_built)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret = 'size_t' if name.endswith('_workspace') else 'int'
        decl = re.search(r'\b%s\s+%s\(([^;]*)\);' % (ret, name), code)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES['ggan_mix_rbf_sums_workspace'][0] is C.c_size_t
    assert 'mmd.py:20-67' in hdr                                   # the reference call site
    assert 'mmd_sets.hip' in build.SOURCES
    # the old pair keeps its signatures, the ABI version its value
    assert len(_lib.SIGNATURES['ggan_mix_rbf_mmd2_fwd'][1]) == 11 and len(_lib.SIGNATURES['ggan_mix_rbf_mmd2_bwd'][1]) == 12
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800
    assert '#define GGAN_ABI_VERSION 800' in hdr


def test_workspace_is_linear_in_the_rows(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    w = L.ggan_mix_rbf_sums_workspace
    assert w(1, 1) >= 4 * 2 + 24
    sizes = [(1, 1), (130, 67), (10000, 10000), (65536, 65536), (131072, 131072)]
    for m, n in sizes:
        assert 0 < w(m, n) <= 64 * 1024 + 64 * (m + n), (m, n, w(m, n))        # a constant + a few bytes per row: never (m + n)^2
    assert w(131072, 131072) < 2 * w(65536, 65536) + 64 * 1024
    assert w(0, 5) == 0 and w(5, 131073) == 0


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)
    sg = (C.c_float * 3)(2., 5., 10.)
    big = 1 << 20

    def call(X=p(), Y=p(), m=8, n=8, d=4, s=sg, wt=None, ns=3, out=p(), ws=p(), wsb=big):
        rc = L.ggan_mix_rbf_sums(X, Y, m, n, d, s, wt, ns, out, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(X=None), 'null'), (dict(Y=None), 'null'), (dict(s=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'),
                     (dict(ns=0), 'ns'), (dict(ns=9), 'ns'), (dict(d=0), 'd < 1'), (dict(m=0), 'm, n'), (dict(n=131073), 'm, n'),
                     (dict(wsb=L.ggan_mix_rbf_sums_workspace(8, 8) - 1), 'workspace'), (dict(wsb=0), 'workspace')):
        rc, msg = call(**kw)
        assert rc < 0 and 'ggan_mix_rbf_sums' in msg and word in msg, (kw, rc, msg)
    # the two new entry points of the fused op: the old limits, and two rows per set
    for name in ('ggan_mix_rbf_mmd2_unbiased_fwd', 'ggan_mix_rbf_mmd2_unbiased_bwd'):
        tail = (p(), p(), None) if name.endswith('fwd') else (p(), p(), p(), None)
        for m, n, ns in ((1, 8, 3), (8, 1, 3), (300, 300, 3), (8, 8, 9)):
            assert getattr(L, name)(p(), p(), m, n, 4, sg, None, ns, *tail) < 0, (name, m, n, ns)
            assert name in L.ggan_last_error().decode()


def test_python_ops_refuse_what_they_cannot_do(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    from graphical_gan_amd import tflib as lib
    x, y = torch.zeros(4, 3), torch.zeros(5, 3)
    with pytest.raises(_lib.GganError):
        F.mix_rbf_sums(x, y, R.SIGMAS)                               # no CPU path
    with pytest.raises(_lib.GganError):
        F.mix_rbf_sums(x.requires_grad_(True), y, R.SIGMAS)          # no backward
    for m, n in ((1, 5), (5, 1)):
        with pytest.raises(ValueError):
            lib.objs.mmd.mix_rbf_mmd2(torch.zeros(m, 3), torch.zeros(n, 3), biased=False)
    with pytest.raises(ValueError):                                  # beyond the fused op's rows there is no gradient to offer
        lib.objs.mmd.mix_rbf_mmd2(torch.zeros(400, 3, requires_grad=True), torch.zeros(200, 3))


SCORE_VARS = ['GGAN_%s_EVERY' % n for n in ('MMD', 'PRDC', 'KNN', 'PARZEN', 'REC')]


def test_mmd_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    for v in SCORE_VARS:
        monkeypatch.delenv(v, raising=False)
    base_eval = {s: run.eval_settings(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    base_man = {s: run.manifold_settings(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {} and run.score_settings('/somewhere/%s.py' % s) == {}
    monkeypatch.setenv('GGAN_MMD_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.score_settings(s) == {'MMD_EVERY': 20} and run.score_settings('/somewhere/%s.py' % s) == {'MMD_EVERY': 20}
    for s in SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {}
    # the other settings functions do not learn the variable, and the key is no EVAL_KEY
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:
        assert run.eval_settings(s) == base_eval[s] and run.manifold_settings(s) == base_man[s]
        assert 'MMD_EVERY' not in run.eval_settings(s)
    assert 'MMD_EVERY' not in run.EVAL_KEYS and 'MMD_EVERY' not in run.MANIFOLD_KEYS
    S = dict(run.reference_block('gan_inference_cifar10'), **run.score_settings('gan_inference_cifar10'))
    assert run.eval_plan(S) is None and run.manifold_plan(S) is None
    assert [it for it in range(60) if 'mmd' in run.scores_due(S, it)] == [19, 39, 59]
    assert all(run.scores_due(S, it) in ((), ('mmd',)) for it in range(60))              # no other score fires
    assert not any(run.scores_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_all_five_switches_at_once(monkeypatch):
    """distinct values: an image script gets the five keys with their own values, a state-space script REC_EVERY alone, and where several
    cadences coincide scores_due names them in the table's order"""
    from graphical_gan_amd import run
    for v, n in zip(SCORE_VARS, (2, 3, 4, 6, 12)):
        monkeypatch.setenv(v, str(n))
    want = dict(MMD_EVERY=2, PRDC_EVERY=3, KNN_EVERY=4, PARZEN_EVERY=6, REC_EVERY=12)
    for s in IMAGE_SCRIPTS:
        assert run.score_settings(s) == want and list(run.score_settings(s)) == list(want)
    for s in SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {'REC_EVERY': 12}
    assert run.score_settings('no_such_script') == {}
    assert run.scores_due(want, 11) == ('mmd', 'prdc', 'knn', 'parzen', 'rec')
    assert run.scores_due(want, 5) == ('mmd', 'prdc', 'parzen') and run.scores_due(want, 3) == ('mmd', 'knn')
    assert run.scores_due(want, 1) == ('mmd',) and run.scores_due(want, 0) == () and run.scores_due(want, 2) == ('prdc',)
    assert run.scores_due(dict(reversed(list(want.items()))), 11) == ('mmd', 'prdc', 'knn', 'parzen', 'rec')      # (the table's order, not the block's)


def test_the_ten_scripts_carry_the_line():
    """each script carries the score_settings line exactly once and names no per-score settings function (which script gets which score:
    the score_settings tests)"""
    line = 'SETTINGS.update(run.score_settings(__file__))'
    seen = {}
    for path in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py')):
        text = open(path).read()
        seen[os.path.splitext(os.path.basename(path))[0]] = text.count(line)
        assert not re.search(r'(mmd|prdc|knn|parzen|rec)_(settings|due)', text), path
    assert sorted(seen) == sorted(IMAGE_SCRIPTS + SEQUENCE_SCRIPTS)
    assert all(n == 1 for n in seen.values()), seen


def test_the_table_and_its_keywords(monkeypatch):
    """the five scores are rows of one table, in the logged order; each is off unless asked for, by flag or by keyword, and a keyword that
    is no row is refused"""
    from graphical_gan_amd import evaluate
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, 'parse_args', parse)
    for flags in ([], ['--knn']):
        with pytest.raises(SystemExit):
            evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    for r in evaluate.SET_SCORES:
        assert getattr(parsed[0], r.name) is False and getattr(parsed[1], r.name) is (r.name == 'knn'), r.name
    xs = [np.zeros((4, 6), np.float32)]
    ev = object.__new__(evaluate.Evaluator)
    with pytest.raises(ValueError, match='no score was asked for'):
        ev.set_scores(xs)
    with pytest.raises(ValueError, match='no score was asked for'):
        ev.set_scores(xs, mmd=False, rec=False)
    with pytest.raises(TypeError, match='mmd, prdc, knn, parzen, rec'):
        ev.set_scores(xs, fid=True)
    with pytest.raises(TypeError, match='mmd, prdc, knn, parzen, rec'):
        evaluate.evaluate_once(None, {}, fid=True)


def test_evaluate_once_and_cli_default_to_no_mmd():
    from graphical_gan_amd import evaluate
    assert hasattr(evaluate.Evaluator, 'mmd_scores') and evaluate.MMD_MAX_ROWS == 10000
    with pytest.raises(SystemExit):            # refused before anything is built
        evaluate.main(['nowhere.npz', '--script', 'ssgan_inference_chairs', '--out-dir', 'x', '--mmd'])


def test_restatement_against_the_oracle_and_the_formula():
    from oracle import objs as J, tape as tp
    rng = np.random.default_rng(3)
    m, n, d = 5, 9, 16
    x, y = rng.standard_normal((m, d)) * 1.5, rng.standard_normal((n, d)) + 0.3
    ref_b = float(J.mix_rbf_mmd2(tp.T(x), tp.T(y)).v)
    assert abs(R.mmd2(x, y, biased=True) - ref_b) <= 1e-12 * max(1.0, abs(ref_b))
    assert abs(R.mmd2_direct(x, y, biased=True) - ref_b) <= 1e-12
    s = R.sums3(x, y)
    want_u = s[0] / (m * (m - 1)) + s[1] / (n * (n - 1)) - 2 * s[2] / (m * n)
    assert abs(R.mmd2(x, y, biased=False) - want_u) <= 1e-15
    assert abs(R.mmd2_direct(x, y, biased=False) - want_u) <= 1e-12
    assert abs(want_u - ref_b) > 1e-3                                 # (the two estimators differ visibly at this size)
    # weights: the constant diagonal is sum(wts)
    w = (1., 2., 4.)
    for biased in (True, False):
        assert abs(R.mmd2(x, y, R.SIGMAS[:3], w, biased) - R.mmd2_direct(x, y, R.SIGMAS[:3], w, biased)) <= 1e-12
    # the package's own host formula is the same one
    from graphical_gan_amd import functional as F
    for biased in (True, False):
        assert abs(float(F.mmd2_from_sums(s, m, n, 6.0, biased)) - R.from_sums(s, m, n, 6.0, biased)) <= 1e-15
