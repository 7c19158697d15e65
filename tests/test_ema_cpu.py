"""not-gpu: the weight average's ABI (header, binding, built library, argument errors without a GPU), its two settings for all ten scripts,
the CLI flag, and the float64 restatement of the recurrence the GPU tests measure against: its closed form on constant weights and the
update ordinals at which TensorFlow's warm-up branch (1 + t) / (10 + t) hands over to the decay."""
import ctypes as C
import glob
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_ema_step', 'ggan_swap')
SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')] + \
          ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']


# ---- the restatement (tf.train.ExponentialMovingAverage(decay, num_updates), as TensorFlow 1 documents it) -----------------------------
def ema_decay_at(decay, t):
    """d_t = min(decay, (1 + t) / (10 + t)), t = ordinal of the update just applied (1, 2, ...); float64"""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def ema_ref(shadow, theta, decay, t):
    """shadow - (1 - d_t) * (shadow - theta) in float64"""
    shadow, theta = np.asarray(shadow, np.float64), np.asarray(theta, np.float64)
    return shadow - (1.0 - ema_decay_at(decay, t)) * (shadow - theta)


def test_constant_weights_closed_form():
    rng = np.random.default_rng(0)
    c, s0 = rng.standard_normal(17), rng.standard_normal(17)
    for decay in (0.9, 0.999, 0.0):
        s, prod = s0.copy(), 1.0
        for t in range(1, 200):
            s = ema_ref(s, c, decay, t)
            prod *= ema_decay_at(decay, t)
            assert np.allclose(s, c + (s0 - c) * prod, rtol=0, atol=1e-14), (decay, t)
    assert np.allclose(ema_ref(s0, c, 0.0, 5), c, rtol=0, atol=1e-15)      # decay 0: the average is the last iterate


def test_warm_up_hands_over_to_the_decay():
    """(1 + t) / (10 + t) reaches 0.9 at t = 80 (81 / 90, exactly) and 0.999 at t = 8990 (8991 / 9000)"""
    for decay, at in ((Fraction(9, 10), 80), (Fraction(999, 1000), 8990)):
        warm = lambda t: Fraction(1 + t, 10 + t)
        assert warm(at) == decay and warm(at - 1) < decay < warm(at + 1)
        d = float(decay)
        assert ema_decay_at(d, at - 1) < d and ema_decay_at(d, at + 1) == d and ema_decay_at(d, 10 ** 6) == d
        assert abs(ema_decay_at(d, at) - d) <= 2.0 ** -53
        assert ema_decay_at(d, 1) == 2.0 / 11.0
    assert 81.0 / 90.0 == 0.9


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(lib_built):
    from graphical_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = C.CDLL(lib_built)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r'\bint\s+%s\(([^;]*)\);' % name, code)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is C.c_int, name
    assert _lib.SIGNATURES['ggan_ema_step'][1][2:5] == [C.c_size_t, C.c_void_p, C.c_float]
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800            # new entry points only
    assert '#define GGAN_ABI_VERSION 800' in hdr
    assert 'ExponentialMovingAverage' in hdr and 'NO call site in the reference' in hdr


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)

    def ema(shadow=p(4096), theta=p(1 << 20), n=64, step=p(1 << 21), decay=0.9):
        rc = L.ggan_ema_step(shadow, theta, n, step, decay, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(shadow=None), 'null'), (dict(theta=None), 'null'), (dict(step=None), 'null'), (dict(decay=1.0), 'decay'),
                     (dict(decay=-0.1), 'decay'), (dict(decay=1.5), 'decay'), (dict(decay=float('nan')), 'decay'),
                     (dict(theta=p(4096)), 'same buffer'), (dict(shadow=p(4100)), 'aligned'),
                     (dict(theta=p(4096 + 4 * 63)), 'overlap'), (dict(shadow=p(4096 + 4 * 63), theta=p(4096)), 'overlap'),
                     (dict(theta=p(4096 + 16)), 'overlap')):
        rc, msg = ema(**kw)
        assert rc == -1 and 'ggan_ema_step' in msg and word in msg, (kw, rc, msg)

    def swap(a=p(4096), b=p(1 << 20), n=64):
        rc = L.ggan_swap(a, b, n, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(a=None), 'null'), (dict(b=None), 'null'), (dict(b=p(4096)), 'overlap'), (dict(b=p(4096 + 4 * 63)), 'overlap'),
                     (dict(a=p(4096 + 4 * 63), b=p(4096)), 'overlap'), (dict(a=p(4100)), 'aligned')):
        rc, msg = swap(**kw)
        assert rc == -1 and 'ggan_swap' in msg and word in msg, (kw, rc, msg)
    assert ema(n=0)[0] == 0 and swap(n=0)[0] == 0                           # nothing to do is no error (and no launch)


def test_python_ops_and_optimizer_refuse_bad_arguments(lib_built):
    import torch
    from graphical_gan_amd import functional as F, optim, _lib
    a, b, step = torch.zeros(8), torch.zeros(8), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.GganError, match='no CPU path'):           # a missing kernel is an error, not a fall-back
        F.ema_step_(a, b, step, 0.5)
    with pytest.raises(_lib.GganError, match='no CPU path'):
        F.swap_(a, b)
    with pytest.raises(AssertionError):
        F.ema_step_(a, b, step.long(), 0.5)
    with pytest.raises(AssertionError):
        F.swap_(a, torch.zeros(9))
    for bad in (1.0, -0.5, 2, float('nan')):
        with pytest.raises(ValueError):
            optim.check_ema_decay(bad)
    assert optim.check_ema_decay(0) == 0.0 and optim.check_ema_decay('0.999') == 0.999


# ---- settings --------------------------------------------------------------------------------------------------------------------------
def test_ema_settings(monkeypatch):
    from graphical_gan_amd import run
    for v in ('GGAN_EMA_DECAY', 'GGAN_EMA_EVAL'):
        monkeypatch.delenv(v, raising=False)
    for s in SCRIPTS:                                  # the default is off
        assert run.ema_settings(s) == {} and run.ema_settings('/somewhere/%s.py' % s) == {}
        assert run.ema_passes(run.reference_block(s)) == ('live',)
    monkeypatch.setenv('GGAN_EMA_DECAY', '0.999')
    for s in SCRIPTS:                                  # all ten scripts
        assert run.ema_settings(s) == {'EMA_DECAY': 0.999, 'EMA_EVAL': 'live'}
    assert run.ema_settings('no_such_script') == {}
    for which, passes in (('live', ('live',)), ('ema', ('ema',)), ('both', ('live', 'ema'))):
        monkeypatch.setenv('GGAN_EMA_EVAL', which)
        S = run.ema_settings('ssgan_inference_chairs')
        assert S == {'EMA_DECAY': 0.999, 'EMA_EVAL': which} and run.ema_passes(S) == passes
    monkeypatch.setenv('GGAN_EMA_DECAY', '0')
    assert run.ema_settings(SCRIPTS[0])['EMA_DECAY'] == 0.0
    for bad in ('1', 'x', '-0.1', '1.5', 'nan'):
        monkeypatch.setenv('GGAN_EMA_DECAY', bad)
        with pytest.raises(ValueError, match='EMA_DECAY'):
            run.ema_settings(SCRIPTS[0])
    monkeypatch.setenv('GGAN_EMA_DECAY', '0.9')
    monkeypatch.setenv('GGAN_EMA_EVAL', 'foo')
    with pytest.raises(ValueError, match='EMA_EVAL'):
        run.ema_settings(SCRIPTS[0])
    monkeypatch.delenv('GGAN_EMA_DECAY')
    monkeypatch.setenv('GGAN_EMA_EVAL', 'ema')
    with pytest.raises(ValueError, match='needs GGAN_EMA_DECAY'):     # nothing to score without an average
        run.ema_settings(SCRIPTS[0])
    with pytest.raises(ValueError, match='needs EMA_DECAY'):
        run.ema_check({'EMA_EVAL': 'both'})
    assert run.ema_check({}) == {} and run.ema_check({'EMA_EVAL': 'live'}) == {}


def test_the_ten_scripts_carry_the_line():
    line = 'SETTINGS.update(run.ema_settings(__file__))'
    seen = {}
    for path in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py')):
        seen[os.path.splitext(os.path.basename(path))[0]] = open(path).read().count(line)
    assert sorted(seen) == sorted(SCRIPTS)
    assert all(seen[s] == 1 for s in seen), seen


def test_cli_accepts_ema_and_names_the_missing_keys(monkeypatch, capsys, tmp_path):
    from graphical_gan_amd import evaluate, engine, checkpoint

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(engine, 'Trainer', stop)            # (what main builds once no argument has been refused)
    monkeypatch.setattr(evaluate.lib, 'get_device', stop)
    plain = str(tmp_path / 'plain.npz')
    np.savez(plain, **{'Generator.Input.W': np.zeros((2, 2), np.float32), 'adam/gen/step': np.zeros(1, np.int32)})
    with pytest.raises(SystemExit):                         # a checkpoint of a run that did not average: said before anything is built
        evaluate.main([plain, '--script', 'gan_inference_cifar10', '--ema'])
    err = capsys.readouterr().err
    assert '--ema' in err and 'ema/gen/<param name>' in err and 'ema/gen/decay' in err
    with pytest.raises(ValueError, match='ema/gen/decay'):
        checkpoint.ema_params(plain)
    avg = str(tmp_path / 'avg.npz')
    np.savez(avg, **{'Generator.Input.W': np.zeros((2, 2), np.float32), 'ema/gen/Generator.Input.W': np.ones((2, 2), np.float32),
                     'ema/gen/decay': np.asarray(0.9)})
    got = checkpoint.ema_params(avg)
    assert list(got) == ['Generator.Input.W'] and np.array_equal(got['Generator.Input.W'], np.ones((2, 2), np.float32))
    with pytest.raises(Reached):                            # ... and one that did is accepted
        evaluate.main([avg, '--script', 'gan_inference_cifar10', '--ema'])
    with pytest.raises(Reached):
        evaluate.main([plain, '--script', 'gan_inference_cifar10'])


def test_names_and_files_of_an_evaluator_on_averaged_weights():
    from graphical_gan_amd import evaluate
    ev = evaluate._Passes()
    assert ev.weights == 'live' and ev.tag({'dev gen cost': 1.0}) == {'dev gen cost': 1.0} and ev._fname('a/b_5.png') == 'a/b_5.png'
    ev.weights = 'ema'
    assert ev.tag({'dev gen cost': 1.0, 'dev rec mse x': 2.0}) == {'dev gen cost ema': 1.0, 'dev rec mse x ema': 2.0}
    assert ev._fname('a/b_5.png') == 'a/b_5_ema.png' and ev._fname('x.y/samples_eval.gif') == 'x.y/samples_eval_ema.gif'
