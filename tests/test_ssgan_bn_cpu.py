"""BN_FLAG of the state-space scripts (ssgan_inference_moving_mnist.py:31-34, ssgan_inference_chairs.py:33-37), host side:
run.config's flags, and the self-consistency of tests/golden/reference_trace_ssgan_bn.json (its generator re-run when the reference
is on this machine)."""
import json
import os
import subprocess
import sys

import pytest

from graphical_gan_amd import run

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'reference_trace_ssgan_bn.json')
SCRIPTS = ('ssgan_inference_moving_mnist', 'ssgan_inference_chairs')


@pytest.mark.parametrize('script', SCRIPTS)
def test_bn_flags_default_off(script):
    cfg = run.config(run.reference_block(script))
    assert (cfg.bn_g, cfg.bn_e, cfg.bn_d) == (False, False, False)


@pytest.mark.parametrize('script', SCRIPTS)
def test_bn_flag_sets_every_child(script):
    cfg = run.config(run.reference_block(script, BN_FLAG=True))
    assert (cfg.bn_g, cfg.bn_e, cfg.bn_d) == (True, True, True)


@pytest.mark.parametrize('child', ['BN_FLAG_G', 'BN_FLAG_E', 'BN_FLAG_D'])
def test_each_child_flag_alone(child):
    cfg = run.config(run.reference_block('ssgan_inference_moving_mnist', **{child: True}))
    assert (cfg.bn_g, cfg.bn_e, cfg.bn_d) == tuple(c == child for c in ('BN_FLAG_G', 'BN_FLAG_E', 'BN_FLAG_D'))
    cfg = run.config(run.reference_block('ssgan_inference_moving_mnist', BN_FLAG=True, **{child: False}))
    assert (cfg.bn_g, cfg.bn_e, cfg.bn_d) == tuple(c != child for c in ('BN_FLAG_G', 'BN_FLAG_E', 'BN_FLAG_D'))


def test_bn_flag_op_has_no_effect():
    """ssgan_inference_chairs.py:37: no net of the reference reads BN_FLAG_OP"""
    a = run.config(run.reference_block('ssgan_inference_chairs'))
    b = run.config(run.reference_block('ssgan_inference_chairs', BN_FLAG_OP=True))
    assert vars(a) == vars(b)


def test_3dcnn_config_with_bn():
    cfg = run.config(run.reference_block('ssgan_inference_moving_mnist', MODE='ali', ALI_MODE='3dcnn', BN_FLAG=True))
    assert (cfg.seq_critic, cfg.ali_mode, cfg.bn_d) == (True, '3dcnn', True)


def _fixture():
    return json.load(open(FIXTURE))


def test_fixture_parameters_are_the_reference_batchnorm_layers():
    """every BatchNorm parameter the fixture recorded sits where the reference scripts place one, with the reference's shape: [1, F]
    for Generator.BN1 (axes [0]), [C] + moving statistics for the [0,2,3] layers, [1,1,1,1,C] and no moving statistics for the
    3dcnn critic's [0,1,2,3] layers"""
    T = _fixture()
    assert len(T) == 6
    for key, t in T.items():
        shapes = dict(zip(t['names'], t['shapes']))
        c = dict(t['script_constants'], **t['constants'])
        assert c['BN_FLAG'] is True, key
        d = c['DIM']
        bn = {n: s for n, s in shapes.items() if '.BN' in n}
        assert shapes['Generator.BN1.scale'] == shapes['Generator.BN1.offset'] == [1, 4 * 4 * 8 * d]
        assert 'Generator.BN1.moving_mean' not in shapes
        for i, ch in ((2, 4 * d), (3, 2 * d), (4, d)):
            for suf in ('offset', 'scale', 'moving_mean', 'moving_variance'):
                assert shapes['Generator.BN%d.%s' % (i, suf)] == [ch], (key, i, suf)
        for i, ch in ((2, 2 * d), (3, 4 * d), (4, 8 * d)):
            for pre in ('Extractor', 'Extractor.G'):
                assert shapes['%s.BN%d.scale' % (pre, i)] == [ch], (key, pre, i)
            if t['ali_mode'] == '3dcnn':
                assert shapes['Discriminator.BN%d.scale' % i] == shapes['Discriminator.BN%d.offset' % i] == [1, 1, 1, 1, ch]
                assert 'Discriminator.BN%d.moving_mean' % i not in shapes
            else:
                assert shapes['Discriminator.BN%d.moving_variance' % i] == [ch], (key, i)
        n_5d = 6 if t['ali_mode'] == '3dcnn' else 0
        assert sorted(t['bn_5d']) == sorted(n for n in bn if len(bn[n]) == 5) and len(t['bn_5d']) == n_5d, key
        # 1 + 3 generator layers, 2 x 3 extractor layers, 3 critic layers
        assert len({n.rsplit('.', 1)[0] for n in bn}) == 13, (key, sorted(bn))


def test_fixture_records_the_loop_of_every_case():
    for key, t in _fixture().items():
        runs = [r for r in t['runs'] if r['train']]
        assert len(runs) >= t['constants']['ITERS'], key       # (the training runs of the loop: critic and generator steps)
        assert t['first_grads'] and len(t['first_grads']) == len(t['names']) == len(t['final']), key


def _reference_dir():
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    try:
        import make_reference_trace as MRT
        return MRT.REF
    finally:
        sys.path.pop(0)


def test_generator_reproduces_the_fixture(tmp_path):
    import shutil
    if not os.path.isdir(_reference_dir()):
        pytest.skip('the reference scripts are not on this machine')
    gen = os.path.join(HERE, 'golden', 'make_ssgan_bn_trace.py')
    work = tmp_path / 'golden'
    shutil.copytree(os.path.join(HERE, 'golden'), work, ignore=shutil.ignore_patterns('*.npz', 'reference_trace*.json'))
    root = os.path.dirname(HERE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    subprocess.check_call([sys.executable, str(work / os.path.basename(gen))], cwd=root, env=env, stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    assert json.load(open(work / 'reference_trace_ssgan_bn.json')) == _fixture()
