"""not-gpu: the Parzen-window op's ABI (header, binding, built library, argument errors without a GPU), what the Python ops refuse, the
cadence settings of the dev-set Parzen pass, what the pass refuses before any device work, and the float64
restatement tests/_parzen_ref.py: its known answers by hand and the conditions on the shared cases under which the GPU tests test
something (a dropped candidate shows; an unshifted sum is log 0)."""
import contextlib
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parzen_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_parzen_lse_workspace', 'ggan_parzen_lse')
IMAGE_SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')]
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
SCORE_VARS = ['GGAN_%s_EVERY' % n for n in ('MMD', 'PRDC', 'KNN', 'PARZEN', 'REC')]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_restatement_known_answers_by_hand():
    q = np.array([[0.0, 0.0]])
    one = R.lse(q, np.array([[3.0, 4.0]]), [0.5, 2.0])                      # one candidate at D = 25: -D / (2 sigma^2)
    assert np.allclose(one[:, 0], [-50.0, -3.125], rtol=0, atol=1e-13)
    two = R.lse(q, np.array([[3.0, 4.0], [-4.0, 3.0]]), [0.5, 2.0])         # two at equal distance: log 2 - D / (2 sigma^2)
    assert np.allclose(two[:, 0], [np.log(2) - 50.0, np.log(2) - 3.125], rtol=0, atol=1e-13)
    dup = R.lse(q, np.array([[0.0, 0.0], [30.0, 40.0]]), [0.5, 1e3])        # a duplicate of the query: log(1 + exp(-2500 / (2 sigma^2)))
    assert dup[0, 0] == 0.0 and abs(dup[1, 0] - np.log1p(np.exp(-1.25e-3))) < 1e-15
    far = R.lse(q, np.array([[300.0, 400.0], [300.0, 401.0]]), [0.1])       # exponents ~ -1.25e7: the plain sum is log 0, the shifted one is not
    assert np.isneginf(R.plain_lse(R.d2(q, [[300.0, 400.0], [300.0, 401.0]]), [0.1])[0, 0])
    assert abs(far[0, 0] - (-250000.0 * 50.0)) < 1e-6                        # (the second candidate's term, exp(-801 * 50), is 0)
    # the unit-scale density: a set scaled by 2 with the bandwidth scaled by 2 has the same log-likelihood (the Jacobian is in the formula)
    rng = np.random.default_rng(3)
    a, b = rng.random((5, 4)), rng.random((7, 4))
    assert np.allclose(R.ll(2 * a - 1, 2 * b - 1, [0.3, 1.0], scale=2.0), R.ll(a, b, [0.3, 1.0]), rtol=0, atol=1e-12)
    # one dimension, one candidate: the log of the normal density itself
    assert abs(R.ll([[0.5]], [[0.2]], [0.3])[0, 0] - (-0.5 * np.log(2 * np.pi * 0.09) - 0.09 / 0.18)) < 1e-14
    # the pass: 4 minibatches of 2 -> 4 validation rows (half the minibatches), the first of equal validation means, population std
    assert [R.valid_rows(r, 2) for r in (4, 6, 8, 4000)] == [2, 2, 4, 1000] and R.valid_rows(64, 8, valid=20) == 16
    p = R.pass_values(a[:4], b[:4], 2, sigmas=[0.5, 0.5, 0.1])
    assert p['best'] == 0 and p['v'] == 2 and p['count'] == 2 and p['sigma'] == 0.5
    held = R.ll(a[2:4], b[:4], [0.5])[0]
    assert abs(p['ll'] - held.mean()) < 1e-13 and abs(p['se'] - abs(held[0] - held[1]) / 2 / np.sqrt(2)) < 1e-13


@pytest.mark.parametrize('m,n,d', [c for c in R.LATTICE_CASES if c[1] >= 67])
def test_a_dropped_candidate_shows_on_the_lattice_cases(m, n, d):
    """a condition on the inputs, from the reference alone: at the largest bandwidth every candidate counts, so a kernel that lost the
    last one would be off by at least 10 gates in EVERY row"""
    Q, S, sig = R.lattice(m, n, d)
    assert Q.dtype == np.float32 and not Q.flags.writeable and R.lattice(m, n, d)[0] is Q
    assert np.array_equal(Q, np.round(Q)) and np.abs(Q).max() == 2 and np.allclose(sig, np.array([0.05, 0.2, 1, 30]) * np.sqrt(4 * d))
    D, ref = R.case_d2(m, n, d), R.reference(m, n, d)
    assert int((D == 0).sum()) >= min(m, n) // 3                            # the planted copies: exact zeros
    moved = np.abs(R.lse_from_d2(D[:, :-1], sig[-1:]) - ref[-1:]) / R.gate(ref[-1:])
    print((m, n, d), 'a dropped candidate moves the widest column by', moved.min(), '...', moved.max(), 'gates')
    assert moved.min() >= 10.0


@pytest.mark.parametrize('m,n,d', R.IMAGE_CASES)
def test_an_unshifted_sum_is_log_zero_on_the_image_like_cases(m, n, d):
    Q, S, sig = R.image_like(m, n, d)
    assert Q.dtype == np.float32 and Q.min() >= (0.0 if d == 784 else -1.0) and Q.max() < 1.0 and len(sig) == 10
    D, ref = R.case_d2(m, n, d), R.reference(m, n, d)
    print((m, n, d), 'reference from', ref.min(), 'to', ref.max())
    assert np.all(np.isfinite(ref)) and ref.min() < -1000.0
    assert np.all(np.isneginf(R.plain_lse(D, sig[:1])))


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
    assert 'parzen_sets.hip' in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'parzen_sets.hip'))
    assert '#define GGAN_PARZEN_MAX_SIGMAS 16' in hdr
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800            # new entry points only
    assert '#define GGAN_ABI_VERSION 800' in hdr


def test_workspace(lib_built):
    from graphical_gan_amd import _lib
    w = _lib.load().ggan_parzen_lse_workspace
    assert w(1, 1, 1) >= 4 * 2 + 4 * 2
    for m, n in ((2, 2), (130, 300), (10000, 10000), (131072, 131072), (1, 131072), (131072, 1)):
        rows = (2048 + (m + 127) // 128) * 128             # partials: about 2048 workgroups of 128 query rows each -- never m n
        for ns in (1, 10, 16):
            assert 0 < w(m, n, ns) <= 32 + 4 * (m + n) + 4 * (1 + ns) * rows, (m, n, ns, w(m, n, ns))
    assert w(0, 5, 1) == 0 and w(5, 0, 1) == 0 and w(131073, 5, 1) == 0 and w(5, 131073, 1) == 0
    assert w(9, 9, 0) == 0 and w(9, 9, 17) == 0 and w(9, 9, -1) == 0


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)
    big = 1 << 24
    sig = lambda *v: C.cast((C.c_float * len(v))(*v), C.c_void_p)

    def call(Q=p(), S=p(), m=9, n=9, d=4, sigmas=sig(0.5, 1.0), ns=2, lse=p(), ws=p(), wsb=big):
        rc = L.ggan_parzen_lse(Q, S, m, n, d, sigmas, ns, lse, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(Q=None), 'null'), (dict(S=None), 'null'), (dict(sigmas=None), 'null'), (dict(lse=None), 'null'),
                     (dict(ws=None), 'null'), (dict(m=0), 'm, n'), (dict(n=0), 'm, n'), (dict(m=131073), 'm, n'), (dict(n=131073), 'm, n'),
                     (dict(d=0), 'd < 1'), (dict(ns=0), '1 <= ns <= 16'), (dict(ns=17), '1 <= ns <= 16'),
                     (dict(sigmas=sig(0.5, 0.0)), 'sigma'), (dict(sigmas=sig(-1.0, 1.0)), 'sigma'),
                     (dict(sigmas=sig(0.5, float('inf'))), 'sigma'), (dict(sigmas=sig(float('nan'), 1.0)), 'sigma'),
                     (dict(wsb=L.ggan_parzen_lse_workspace(9, 9, 2) - 1), 'workspace'), (dict(wsb=0), 'workspace'),
                     (dict(ws=p(4100)), 'aligned')):
        rc, msg = call(**kw)
        assert rc < 0 and 'ggan_parzen_lse' in msg and word in msg, (kw, rc, msg)


def test_python_ops_refuse_what_they_cannot_do(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert F.PARZEN_MAX_SIGMAS == 16
    x, y = torch.zeros(7, 3), torch.zeros(9, 3)
    for call in (lambda: F.parzen_lse(x, y, [0.5]), lambda: F.parzen_ll(x, y, [0.5], scale=2.0)):
        with pytest.raises(_lib.GganError):                          # no CPU path
            call()
    g = torch.zeros(7, 3, requires_grad=True)
    for call in (lambda: F.parzen_lse(g, y, [0.5]), lambda: F.parzen_lse(x, g, [0.5]), lambda: F.parzen_ll(g, y, [0.5])):
        with pytest.raises(_lib.GganError, match='no backward'):
            call()
    for call in (lambda: F.parzen_lse(x, torch.zeros(9, 4), [0.5]), lambda: F.parzen_lse(torch.zeros(7), y, [0.5]),
                 lambda: F.parzen_lse(x, torch.zeros(9, 3, 1), [0.5]), lambda: F.parzen_lse(x, y, []), lambda: F.parzen_lse(x, y, [0.5] * 17),
                 lambda: F.parzen_lse(x, y, [0.5, 0.0]), lambda: F.parzen_lse(x, y, [-0.5]), lambda: F.parzen_lse(x, y, [float('inf')]),
                 lambda: F.parzen_lse(x, y, np.array([0.5, float('nan')])), lambda: F.parzen_ll(x, y, [0.5] * 17),
                 lambda: F.parzen_ll(x, y, [0.0]), lambda: F.parzen_ll(x, y, [0.5], scale=0.0)):
        with pytest.raises(ValueError):
            call()


# ---- the pass's switches ---------------------------------------------------------------------------------------------------------------
def test_parzen_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    every = IMAGE_SCRIPTS + SEQUENCE_SCRIPTS
    for v in SCORE_VARS:
        monkeypatch.delenv(v, raising=False)
    others = lambda s: (run.eval_settings(s), run.manifold_settings(s))
    base = {s: others(s) for s in every}
    for s in every:
        assert run.score_settings(s) == {} and run.score_settings('/somewhere/%s.py' % s) == {}
    monkeypatch.setenv('GGAN_PARZEN_EVERY', '20')
    for s in IMAGE_SCRIPTS:                    # (exactly the one key: no other score learns the variable)
        assert run.score_settings(s) == {'PARZEN_EVERY': 20} and run.score_settings('/somewhere/%s.py' % s) == {'PARZEN_EVERY': 20}
    for s in SEQUENCE_SCRIPTS:
        assert run.score_settings(s) == {}
    for s in every:                 # the other settings functions do not learn the variable, and the key is in no *_KEYS
        assert others(s) == base[s]
    assert 'PARZEN_EVERY' not in run.EVAL_KEYS and 'PARZEN_EVERY' not in run.MANIFOLD_KEYS
    S = dict(run.reference_block('gan_inference_mnist'), **run.score_settings('gan_inference_mnist'))
    assert run.eval_plan(S) is None and run.manifold_plan(S) is None
    assert [it for it in range(60) if 'parzen' in run.scores_due(S, it)] == [19, 39, 59]
    assert not any(set(run.scores_due(S, it)) & {'mmd', 'prdc', 'knn'} for it in range(60))
    assert all(run.scores_due(S, it) in ((), ('parzen',)) for it in range(60))           # no other score fires
    assert not any(run.scores_due(run.reference_block('gan_inference_mnist'), it) for it in range(60))
    monkeypatch.delenv('GGAN_PARZEN_EVERY')
    monkeypatch.setenv('GGAN_KNN_EVERY', '20')
    for s in every:
        assert 'PARZEN_EVERY' not in run.score_settings(s)


def test_evaluate_once_and_cli_default_to_no_parzen():
    from graphical_gan_amd import evaluate
    assert evaluate.PARZEN_MAX_ROWS == 10000 and evaluate.PARZEN_VALID_ROWS == 1000
    assert np.array_equal(evaluate.PARZEN_SIGMAS, np.logspace(-1, 0, 10)) and np.array_equal(evaluate.PARZEN_SIGMAS, R.SIGMAS)
    with pytest.raises(SystemExit):            # refused before anything is built
        evaluate.main(['nowhere.npz', '--script', 'ssgan_inference_chairs', '--out-dir', 'x', '--parzen'])


def _bare_evaluator(settings):
    """an Evaluator without a model behind it: enough for what parzen_scores checks before any device work"""
    import torch
    from graphical_gan_amd import evaluate
    ev = object.__new__(evaluate.Evaluator)
    ev.S, ev.device = settings, torch.device('cpu')
    ev.cfg = types.SimpleNamespace(B=4, dataset='mnist', dim_latent=3, output_dim=6, K=0, agg=False, out_act='sigmoid')
    ev.model = types.SimpleNamespace(single_stream=contextlib.nullcontext)
    return ev


def test_parzen_scores_needs_two_minibatches_and_a_legal_grid():
    rng = np.random.default_rng(0)
    xs = [rng.random((4, 6), dtype=np.float32) for _ in range(3)]
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match='at least 2 full minibatches'):
        _bare_evaluator({}).parzen_scores(xs[:1])
    with pytest.raises(ValueError, match='at least 2 full minibatches'):
        _bare_evaluator({}).parzen_scores([xs[0], xs[1][:3]])                  # (a partial minibatch does not count)
    with pytest.raises(ValueError, match='at least 2 full minibatches'):
        _bare_evaluator(dict(PARZEN_MAX_ROWS=7)).parzen_scores(xs)             # rows = 4 < 2 B
    with pytest.raises(ValueError, match='at least 2 full minibatches'):
        _bare_evaluator(dict(PARZEN_MAX_ROWS=7)).set_scores(xs, mmd=True, parzen=True)
    with pytest.raises(ValueError, match='PARZEN_SIGMAS'):
        _bare_evaluator(dict(PARZEN_SIGMAS=np.logspace(-1, 0, 17))).parzen_scores(xs)
    with pytest.raises(ValueError, match='PARZEN_SIGMAS'):
        _bare_evaluator(dict(PARZEN_SIGMAS=[])).parzen_scores(xs)
    assert np.array_equal(np.random.get_state()[1], state)
