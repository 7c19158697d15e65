"""not-gpu: the labelled neighbour-list ops' ABI (header, binding, built library, argument errors without a GPU), what the Python ops
refuse, the cadence settings of the dev-set k-NN accuracy pass, and the float64 restatement tests/_knn_ref.py: its
known answers on a hand-made case and the conditions on the inputs under which the GPU tests' closed-row rule can hide little."""
import contextlib
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_knn_lists_workspace', 'ggan_knn_lists', 'ggan_knn_vote')
IMAGE_SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')]
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
SCORE_VARS = ['GGAN_%s_EVERY' % n for n in ('MMD', 'PRDC', 'KNN', 'PARZEN', 'REC')]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_restatement_known_answers_by_hand():
    """six rows made by hand: rows 1 and 2 are equally far from row 0 (a distance tie), row 3 is a duplicate of row 0, and the labels
    make row 0's k = 2 vote a 1-1 tie"""
    Z = np.array([[0, 0], [1, 0], [-1, 0], [0, 0], [5, 5], [5, 6]], np.float64)
    y = np.array([2, 0, 2, 2, 1, 1])
    # leave-one-out: the duplicate of the query counts, at distance 0; the tie between rows 1 and 2 goes to row 1
    idx, dist = R.lists(Z, Z, 3, skip_diag=True)
    assert idx[0].tolist() == [3, 1, 2] and dist[0].tolist() == [0.0, 1.0, 1.0]
    assert idx[3].tolist() == [0, 1, 2] and idx[1].tolist() == [0, 3, 2] and idx[2].tolist() == [0, 3, 1]
    assert idx[4].tolist() == [5, 1, 0] and idx[5].tolist() == [4, 1, 0]           # |(5,5) - (0,0)|^2 = 50 twice: row 0 before row 3
    assert dist[4].tolist() == [1.0, 41.0, 50.0]
    # not leave-one-out: the query itself is its own nearest candidate, ahead of its duplicate (the lower index)
    assert R.lists(Z, Z, 2)[0][0].tolist() == [0, 3] and R.lists(Z, Z, 2)[0][3].tolist() == [0, 3]
    # votes: k = 1 the duplicate's label; k = 2 labels {2, 0}, a 1-1 tie -> the smallest label; k = 3 labels {2, 0, 2}
    assert R.vote(idx[:, :1], y)[0] == 2 and R.vote(idx[:, :2], y)[0] == 0 and R.vote(idx, y)[0] == 2
    assert R.vote([[0, 1, 2]], [7, 5, 6]).tolist() == [5] and R.vote([[0, 1, 2, 3]], [3, 1, 3, 1]).tolist() == [1]      # 1-1-1 and 2-2
    assert R.vote([[2, 1, 0]], [7, 5, 6]).tolist() == [5]                           # ... whatever the order in the list
    pred = R.vote(idx, y)
    assert pred.tolist() == [2, 2, 2, 2, 0, 0]                                      # (rows 4 and 5: labels {1, 0, 2}, a 1-1-1 tie)
    assert R.accuracy(Z, y, 3) == 0.5
    conf = R.confusion(y, pred, 3)
    assert conf.tolist() == [[0, 0, 1], [2, 0, 0], [0, 0, 3]] and conf.sum() == 6 and np.trace(conf) == 3
    # the closed-row rule on it, with T = 0.4: the band of row 0's 3rd distance (1 +- 0.8) holds rows 1 and 2, labels 0 and 2 -- open both
    # ways; that of row 4's (50 +- 0.8) holds rows 0 and 3, both of label 2 -- an open set, a closed label; row 1's (4 +- 0.8) row 2 alone
    c = R.closed_rows(R.distances(Z, Z, True), 3, np.full(6, 0.4), y)
    assert c['set_closed'].tolist() == [False, True, True, False, False, False]
    assert c['label_closed'].tolist() == [False, True, True, False, True, True]
    assert c['pinned'][1].tolist() == [False, False, True] and not c['pinned'][[0, 3, 4, 5]].any()      # (rows 0 and 3 tie at distance 1)
    lo, hi = R.accuracy_bracket(pred, y, c['label_closed'])
    assert abs(lo - 1.0 / 6.0) < 1e-15 and abs(hi - 0.5) < 1e-15


def test_recipe_is_labelled_and_neither_trivial():
    Z, y = R.labelled(130, 33)
    assert Z.dtype == np.float32 and y.dtype == np.int32 and Z.shape == (130, 33) and sorted(set(y.tolist())) == [0, 1, 2, 3]
    assert R.labelled(130, 33)[0] is Z and not Z.flags.writeable
    Q, yq, Cc, yc = R.split(67, 130, 33)
    assert Q.shape == (67, 33) and Cc.shape == (130, 33) and len(yq) == 67 and len(yc) == 130


# the float cases of tests/test_knn_gpu.py: (m, n, d, leave-one-out, the ks it runs)
FLOAT_CASES = [(5, 9, 16, False, (1, 3)), (67, 130, 33, False, (1, 3, 5)), (130, 130, 33, True, (1, 3, 5, 8)), (257, 300, 131, False, (1, 5, 8)),
               (9, 9, 16, True, (1, 5)), (300, 300, 131, True, (1, 3, 5, 8)), (192, 192, 3072, True, (1, 5)), (160, 192, 3072, False, (1, 5))]


@pytest.mark.parametrize('m,n,d,loo,ks', FLOAT_CASES)
def test_closed_rows_can_hide_little(m, n, d, loo, ks):
    """the GPU tests hold a row to the reference only where float32 cannot decide differently; that only tests something if nearly every
    row is such a row.  Conditions on the INPUTS, from the reference alone: label-open rows at most 2 % for d <= 131 and 10 % at d = 3072."""
    cap = 0.10 if d == 3072 else 0.02
    for k in ks:
        r = R.reference(m, n, d, k, loo)
        label_open, set_open = float(np.mean(~r['label_closed'])), float(np.mean(~r['set_closed']))
        acc = float(np.mean(r['pred'] == r['yq']))
        print((m, n, d, loo), k, 'label-open', label_open, 'set-open', set_open, 'accuracy', acc)
        assert label_open <= cap, (k, label_open)
        assert np.all(r['set_closed'] <= r['label_closed'])                  # a set-closed row is label-closed
        if (n, d) == (130, 33):
            assert label_open == 0.0 and set_open == 0.0
        if d == 3072:
            assert set_open <= 0.25
        if n >= 130:
            assert 0.6 < acc < 0.9                                            # neither trivial end: a wrong vote moves it
            lo, hi = R.accuracy_bracket(r['pred'], r['yq'], r['label_closed'])
            assert lo <= acc <= hi and hi - lo <= cap + 1e-12


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
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
    assert 'knn_lists.hip' in build.SOURCES and 'knn_sets.hip' in build.SOURCES
    assert '#define GGAN_KNN_MAX_K 8' in hdr
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800            # new entry points only
    assert '#define GGAN_ABI_VERSION 800' in hdr


def test_workspace(lib_built):
    from graphical_gan_amd import _lib
    w = _lib.load().ggan_knn_lists_workspace
    assert w(1, 1, 1) >= 4 * 2 + 8
    for m, n in ((2, 2), (130, 300), (10000, 10000), (131072, 131072), (1, 131072)):
        rows = (2048 + (m + 127) // 128) * 128             # partials: about 2048 workgroups of 128 query rows each -- never m n
        assert 0 < w(m, n, min(8, n)) <= 32 + 4 * (m + n) + 8 * 8 * rows, (m, n, w(m, n, min(8, n)))
    assert w(0, 5, 1) == 0 and w(5, 0, 1) == 0 and w(131073, 5, 1) == 0 and w(5, 131073, 1) == 0
    assert w(9, 9, 0) == 0 and w(9, 20, 9) == 0 and w(9, 3, 4) == 0


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)
    big = 1 << 24

    def lists(Q=p(), Cc=p(), m=9, n=9, d=4, k=3, skip=0, idx=p(), d2=None, ws=p(), wsb=big):
        rc = L.ggan_knn_lists(Q, Cc, m, n, d, k, skip, idx, d2, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(Q=None), 'null'), (dict(Cc=None), 'null'), (dict(idx=None), 'null'), (dict(ws=None), 'null'),
                     (dict(k=0), '1 <= k <= 8'), (dict(k=9, n=20), '1 <= k <= 8'), (dict(k=6, n=5), 'k > n - skip_diag'),
                     (dict(k=8, m=8, n=8, skip=1), 'k > n - skip_diag'), (dict(m=8, n=9, skip=1), 'm == n'), (dict(m=0), 'm, n'),
                     (dict(n=131073), 'm, n'), (dict(d=0), 'd < 1'), (dict(wsb=L.ggan_knn_lists_workspace(9, 9, 3) - 1), 'workspace'),
                     (dict(wsb=0), 'workspace'), (dict(ws=p(4100)), 'aligned')):
        rc, msg = lists(**kw)
        assert rc < 0 and 'ggan_knn_lists' in msg and word in msg, (kw, rc, msg)

    def vote(idx=p(), lc=p(), lq=p(), m=9, k=3, classes=4, pred=p(), correct=p(), conf=p()):
        rc = L.ggan_knn_vote(idx, lc, lq, m, k, classes, pred, correct, conf, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(idx=None), 'null'), (dict(lc=None), 'null'), (dict(pred=None), 'null'), (dict(k=0), '1 <= k <= 8'),
                     (dict(k=9), '1 <= k <= 8'), (dict(m=0), 'm'), (dict(classes=1025), 'classes <= 1024'), (dict(classes=0), 'classes'),
                     (dict(lq=None), 'labels_q'), (dict(lq=None, conf=None), 'labels_q')):
        rc, msg = vote(**kw)
        assert rc < 0 and 'ggan_knn_vote' in msg and word in msg, (kw, rc, msg)


def test_python_ops_refuse_what_they_cannot_do(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert F.KNN_MAX_K == 8
    x, y = torch.zeros(7, 3), torch.zeros(9, 3)
    lab = torch.zeros(9, dtype=torch.int32)
    for call in (lambda: F.knn_lists(x, y, 2), lambda: F.knn_accuracy(y, lab, 2, 4), lambda: F.knn_vote(torch.zeros(7, 2, dtype=torch.int32), lab)):
        with pytest.raises(_lib.GganError):                          # no CPU path
            call()
    g = torch.zeros(7, 3, requires_grad=True)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.knn_lists(g, y, 2)
    for call in (lambda: F.knn_lists(x, torch.zeros(9, 4), 2), lambda: F.knn_lists(torch.zeros(7), y, 1), lambda: F.knn_lists(x, y, 0),
                 lambda: F.knn_lists(x, torch.zeros(20, 3), 9), lambda: F.knn_lists(y, x, 8),                   # k > n
                 lambda: F.knn_lists(x, x, 7, skip_diag=True), lambda: F.knn_lists(x, y, 2, skip_diag=True),   # k > n - 1; m != n
                 lambda: F.knn_vote(torch.zeros(7, 2), lab), lambda: F.knn_vote(torch.zeros(7, 9, dtype=torch.int32), lab),
                 lambda: F.knn_accuracy(y, lab, 2, 1025)):
        with pytest.raises(ValueError):
            call()


# ---- the pass's switches ---------------------------------------------------------------------------------------------------------------
def test_knn_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    every = IMAGE_SCRIPTS + SEQUENCE_SCRIPTS
    for v in SCORE_VARS:
        monkeypatch.delenv(v, raising=False)
    base = {s: (run.eval_settings(s), run.manifold_settings(s)) for s in every}
    for s in every:
        assert run.score_settings(s) == {} and run.score_settings('/somewhere/%s.py' % s) == {}
    monkeypatch.setenv('GGAN_KNN_EVERY', '20')
    for s in IMAGE_SCRIPTS:                    # (exactly the one key: no other score learns the variable)
        assert run.score_settings(s) == {'KNN_EVERY': 20} and run.score_settings('/somewhere/%s.py' % s) == {'KNN_EVERY': 20}
    for s in SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {}
    for s in every:                 # the other settings functions do not learn the variable, and the key is in no *_KEYS
        assert (run.eval_settings(s), run.manifold_settings(s)) == base[s]
    assert 'KNN_EVERY' not in run.EVAL_KEYS and 'KNN_EVERY' not in run.MANIFOLD_KEYS
    S = dict(run.reference_block('gan_inference_cifar10'), **run.score_settings('gan_inference_cifar10'))
    assert run.eval_plan(S) is None and run.manifold_plan(S) is None
    assert [it for it in range(60) if 'knn' in run.scores_due(S, it)] == [19, 39, 59]
    assert not any('mmd' in run.scores_due(S, it) or 'prdc' in run.scores_due(S, it) for it in range(60))
    assert all(run.scores_due(S, it) in ((), ('knn',)) for it in range(60))              # no other score fires
    assert not any(run.scores_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))
    monkeypatch.delenv('GGAN_KNN_EVERY')
    monkeypatch.setenv('GGAN_PRDC_EVERY', '20')
    for s in every:
        assert 'KNN_EVERY' not in run.score_settings(s)


def test_evaluate_once_and_cli_default_to_no_knn():
    from graphical_gan_amd import evaluate
    assert evaluate.KNN_MAX_ROWS == 10000 and evaluate.KNN_K == 5
    with pytest.raises(SystemExit):            # refused before anything is built
        evaluate.main(['nowhere.npz', '--script', 'ssgan_inference_chairs', '--out-dir', 'x', '--knn'])


def _bare_evaluator(settings):
    """an Evaluator without a model behind it: enough for what knn_scores checks before any device work"""
    import torch
    from graphical_gan_amd import evaluate
    ev = object.__new__(evaluate.Evaluator)
    ev.S, ev.device = settings, torch.device('cpu')
    ev.cfg = types.SimpleNamespace(B=4, dataset='mnist', dim_latent=3, output_dim=6, K=0, agg=False)
    ev.model = types.SimpleNamespace(single_stream=contextlib.nullcontext)
    return ev


def test_knn_scores_needs_labels_and_a_legal_k():
    rng = np.random.default_rng(0)
    xs = [rng.random((4, 6), dtype=np.float32) for _ in range(3)]
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match='labelled minibatches'):             # (the ValueError cluster_accuracy raises)
        _bare_evaluator({}).knn_scores(xs)
    with pytest.raises(ValueError, match='labelled minibatches'):
        _bare_evaluator({}).knn_scores([(xs[0], np.zeros(4)), xs[1]])
    with pytest.raises(ValueError, match='labelled minibatches'):
        _bare_evaluator({}).set_scores(xs, mmd=True, knn=True)
    for k in (0, 9):
        with pytest.raises(ValueError, match='KNN_K'):
            _bare_evaluator(dict(KNN_K=k)).knn_scores([(x, np.zeros(4)) for x in xs])
    with pytest.raises(ValueError):
        _bare_evaluator({}).set_scores(xs)
    assert np.array_equal(np.random.get_state()[1], state)
