"""not-gpu: the k-NN-ball ops' ABI (header, binding, built library, argument errors without a GPU), what the Python ops refuse, the
cadence settings of the dev-set precision / recall / density / coverage pass, and the float64 restatement
tests/_prdc_ref.py: its known answers, its limiting cases, and the conditions under which the GPU tests' brackets can hide nothing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prdc_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_knn_radii_workspace', 'ggan_knn_radii', 'ggan_ball_counts_workspace', 'ggan_ball_counts')
IMAGE_SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')]
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
SCORE_VARS = ['GGAN_%s_EVERY' % n for n in ('MMD', 'PRDC', 'KNN', 'PARZEN', 'REC')]


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
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    assert 'Kynkaanniemi et al. 2019' in hdr and 'Naeem et al. 2020' in hdr            # what the entries compute
    assert 'knn_sets.hip' in build.SOURCES
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800
    assert '#define GGAN_ABI_VERSION 800' in hdr


def test_workspaces(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    wr, wb = L.ggan_knn_radii_workspace, L.ggan_ball_counts_workspace
    assert wr(2, 1) >= 4 * 2 + 4 * 2 and wb(1, 1) >= 4 * 2 + 8
    for n in (2, 130, 10000, 131072):
        rows = (2048 + (n + 127) // 128) * 128           # partials: about 2048 workgroups of 128 rows each -- never n^2
        assert 0 < wr(n, min(8, n - 1)) <= 16 + 4 * n + 4 * 8 * rows, (n, wr(n, min(8, n - 1)))
        assert 0 < wb(n, n) <= 64 + 8 * n + 8 * rows, (n, wb(n, n))
    assert wr(1, 1) == 0 and wr(9, 0) == 0 and wr(9, 9) == 0 and wr(131073, 1) == 0
    assert wb(0, 5) == 0 and wb(5, 131073) == 0


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)
    big = 1 << 24

    def radii(Z=p(), n=9, d=4, k=3, out=p(), ws=p(), wsb=big):
        rc = L.ggan_knn_radii(Z, n, d, k, out, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(Z=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'), (dict(k=0), 'k'), (dict(k=9, n=20), 'k <= 8'),
                     (dict(k=5, n=5), 'k > n - 1'), (dict(n=0), 'n'), (dict(n=131073), 'n'), (dict(d=0), 'd < 1'),
                     (dict(wsb=L.ggan_knn_radii_workspace(9, 3) - 1), 'workspace'), (dict(wsb=0), 'workspace')):
        rc, msg = radii(**kw)
        assert rc < 0 and 'ggan_knn_radii' in msg and word in msg, (kw, rc, msg)

    def balls(A=p(), B=p(), m=8, n=9, d=4, r=p(), cnt=p(), mn=p(), ws=p(), wsb=big):
        rc = L.ggan_ball_counts(A, B, m, n, d, r, cnt, mn, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(A=None), 'null'), (dict(B=None), 'null'), (dict(r=None), 'null'), (dict(cnt=None), 'null'), (dict(mn=None), 'null'),
                     (dict(ws=None), 'null'), (dict(m=0), 'm, n'), (dict(n=131073), 'm, n'), (dict(d=0), 'd < 1'),
                     (dict(wsb=L.ggan_ball_counts_workspace(8, 9) - 1), 'workspace'), (dict(wsb=0), 'workspace')):
        rc, msg = balls(**kw)
        assert rc < 0 and 'ggan_ball_counts' in msg and word in msg, (kw, rc, msg)


def test_python_ops_refuse_what_they_cannot_do(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    x, y = torch.zeros(7, 3), torch.zeros(9, 3)
    for call in (lambda: F.knn_radii(x, 2), lambda: F.ball_counts(x, y, torch.zeros(9)), lambda: F.prdc(x, y, 2)):
        with pytest.raises(_lib.GganError):                          # no CPU path
            call()
    g = torch.zeros(7, 3, requires_grad=True)
    for call in (lambda: F.knn_radii(g, 2), lambda: F.ball_counts(g, y, torch.zeros(9)), lambda: F.prdc(x, g, 2)):
        with pytest.raises(_lib.GganError, match='no backward'):
            call()
    w = torch.zeros(9, 4)
    for call in (lambda: F.ball_counts(x, w, torch.zeros(9)), lambda: F.prdc(x, w, 2), lambda: F.ball_counts(x, y, torch.zeros(8)),
                 lambda: F.knn_radii(torch.zeros(7), 1),
                 lambda: F.knn_radii(x, 7), lambda: F.knn_radii(x, 0), lambda: F.knn_radii(torch.zeros(20, 3), 9),      # k > n - 1, k < 1, k > 8
                 lambda: F.prdc(x, y, 7), lambda: F.prdc(y, x, 7)):                                                    # k > min(m, n) - 1
        with pytest.raises(ValueError):
            call()


def test_prdc_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    every = IMAGE_SCRIPTS + SEQUENCE_SCRIPTS
    for v in SCORE_VARS:
        monkeypatch.delenv(v, raising=False)
    base = {s: (run.eval_settings(s), run.manifold_settings(s)) for s in every}
    for s in every:
        assert run.score_settings(s) == {} and run.score_settings('/somewhere/%s.py' % s) == {}
    monkeypatch.setenv('GGAN_PRDC_EVERY', '20')
    for s in IMAGE_SCRIPTS:                    # (exactly the one key: no other score learns the variable)
        assert run.score_settings(s) == {'PRDC_EVERY': 20} and run.score_settings('/somewhere/%s.py' % s) == {'PRDC_EVERY': 20}
    for s in SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {}
    # the other settings functions do not learn the variable, and the key is in no *_KEYS
    for s in every:
        assert (run.eval_settings(s), run.manifold_settings(s)) == base[s]
        assert 'PRDC_EVERY' not in run.eval_settings(s)
    assert 'PRDC_EVERY' not in run.EVAL_KEYS and 'PRDC_EVERY' not in run.MANIFOLD_KEYS
    S = dict(run.reference_block('gan_inference_cifar10'), **run.score_settings('gan_inference_cifar10'))
    assert run.eval_plan(S) is None and run.manifold_plan(S) is None
    assert [it for it in range(60) if 'prdc' in run.scores_due(S, it)] == [19, 39, 59]
    assert not any('mmd' in run.scores_due(S, it) for it in range(60))
    assert all(run.scores_due(S, it) in ((), ('prdc',)) for it in range(60))             # no other score fires
    assert not any(run.scores_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))
    # ... and the other way round
    monkeypatch.delenv('GGAN_PRDC_EVERY')
    monkeypatch.setenv('GGAN_MMD_EVERY', '20')
    for s in every:
        assert 'PRDC_EVERY' not in run.score_settings(s)
    assert run.score_settings('gan_inference_cifar10') == {'MMD_EVERY': 20}


def test_evaluate_once_and_cli_default_to_no_prdc():
    from graphical_gan_amd import evaluate
    assert hasattr(evaluate.Evaluator, 'prdc_scores') and evaluate.PRDC_MAX_ROWS == 10000 and evaluate.PRDC_K == 5
    with pytest.raises(SystemExit):            # refused before anything is built
        evaluate.main(['nowhere.npz', '--script', 'ssgan_inference_chairs', '--out-dir', 'x', '--prdc'])


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_restatement_limiting_cases():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((40, 6))
    p, r, d, c = R.prdc(X, X.copy(), 3)                 # the same distinct rows: every row is in its own twin's ball
    assert (p, r, c) == (1.0, 1.0, 1.0) and d > 0
    assert R.prdc(X, X + 1e3, 3) == (0.0, 0.0, 0.0, 0.0)                       # two sets far apart
    A, B = rng.standard_normal((7, 5)), rng.standard_normal((9, 5))
    cnt, mn = R.ball_counts(A, B, np.full(9, 3e38))
    assert cnt.tolist() == [9] * 7 and np.allclose(mn, R.d2(A, B).min(1))
    assert R.ball_counts(A, B, np.full(9, -1.0))[0].tolist() == [0] * 7
    Z = rng.standard_normal((6, 4))
    Z[3] = Z[0]
    Z[5] = Z[0]                                         # three identical rows: a multiset order statistic, self left out by index
    r1, r2, r3 = R.radii(Z, 1), R.radii(Z, 2), R.radii(Z, 3)
    for i in (0, 3, 5):
        assert r1[i] == 0.0 and r2[i] == 0.0 and r3[i] > 0.0
    assert all(r1[i] > 0 for i in (1, 2, 4))
    # inclusive comparisons: a row exactly on a sphere is inside it
    assert R.ball_counts(np.array([[3.0, 4.0]]), np.zeros((1, 2)), [25.0])[0].tolist() == [1]


@pytest.mark.parametrize('shape_k', sorted(R.KNOWN))
def test_restatement_known_answers(shape_k):
    """the values of the recipe (case: generator seeded by the shape; draw order centres, bases, X (mode, t, noise), Y (mode, t, noise),
    Y's off-manifold noise), obtained in float64 and recorded to three decimals"""
    shape, k = shape_k
    got = R.prdc(*R.case(*shape), k)
    print(shape, k, got)
    assert [round(v, 3) for v in got] == list(R.KNOWN[shape_k])
    assert all(0.0 < v < 1.0 for v in got)              # neither trivial end: a wrong count moves them


@pytest.mark.parametrize('shape', R.CASES)
def test_brackets_can_hide_little(shape):
    """the GPU tests accept a count anywhere in [lo, hi]; that only tests something if the bracket is closed for nearly every row"""
    X, Y = R.case(*shape)
    limit = 0.20 if shape[2] == 3072 else 0.01
    for k in (1, 3, 5):
        if k > min(shape[:2]) - 1:
            continue
        for doubled in (True, False):
            amb = R.score_brackets(X, Y, k, doubled)['ambiguous']
            print(shape, k, 'doubled' if doubled else 'single', amb)
            assert amb <= limit, (shape, k, doubled, amb)
