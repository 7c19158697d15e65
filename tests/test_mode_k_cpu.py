"""MODE_K of the mixture scripts beyond CONCRETE (gmgan_inference_cifar10.py:81-86,160-171): the straight-through estimators
STRAIGHT_THROUGHT_CONCRETE and STRAIGHT_THROUGHT -- settings, model configuration, feeds and the C ABI they reach, and the consistency
of the reference fixture tests/golden/reference_trace_mode_k.json (tests/golden/make_mode_k_trace.py)."""
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TRACE = json.load(open(os.path.join(HERE, 'golden', 'reference_trace_mode_k.json')))
STC, ST = 'STRAIGHT_THROUGHT_CONCRETE', 'STRAIGHT_THROUGHT'
SCRIPTS = ('gmgan_inference_mnist', 'gmgan_inference_cifar10', 'gmgan_inference_svhn')


@pytest.mark.parametrize('script', SCRIPTS)
@pytest.mark.parametrize('mode_k', [STC, ST])
def test_config_carries_the_straight_through_mode_k(script, mode_k):
    from graphical_gan_amd import run
    for mode in ('local_ep', 'local_epce'):
        S = run.reference_block(script, MODE=mode, MODE_K=mode_k)
        # the scripts define TEMP for CONCRETE / STRAIGHT_THROUGHT_CONCRETE only (:84-86)
        assert ('TEMP' in S) == (mode_k == STC)
        cfg = run.config(S)
        assert (cfg.mode_k, cfg.mode, cfg.K) == (mode_k, mode, S['N_COMS'])
        if mode_k == STC:
            assert cfg.temp == S['TEMP'] == .1


def test_default_mode_k_and_the_refusals():
    from graphical_gan_amd import run
    from graphical_gan_amd.models import Config
    for script in SCRIPTS:
        S = run.reference_block(script)
        assert S['MODE_K'] == 'CONCRETE' and run.config(S).mode_k == 'CONCRETE'
        # the counterpart script states the reference's switch, at its default
        src = open(os.path.join(ROOT, 'scripts', script + '.py')).read()
        assert re.search(r"^MODE_K = 'CONCRETE'", src, re.M) and 'MODE_K=MODE_K' in src, script
    assert Config('cifar10', n_coms=30).mode_k == 'CONCRETE'
    with pytest.raises(NotImplementedError):
        run.config(run.reference_block('gmgan_inference_cifar10', MODE_K='REINFORCE'))
    # gmgan_inference_face.py hard-codes the CONCRETE branch (:52, :100-104)
    for mk in (STC, ST):
        with pytest.raises(NotImplementedError):
            run.config(run.reference_block('gmgan_inference_face', MODE_K=mk))
    assert run.config(run.reference_block('gmgan_inference_face')).mode_k == 'CONCRETE'
    with pytest.raises(ValueError):
        run.config(run.reference_block('gmgan_inference_mnist', MODE_K='STRAIGHT_THROUGH'))      # (the reference spells it THROUGHT)


@pytest.mark.parametrize('mode_k', ['CONCRETE', STC, ST])
def test_feeds_and_noise_of_each_mode(mode_k):
    """STRAIGHT_THROUGHT draws no Gumbel noise: no buffer, no slot in the noise launch (later draws keep their place)"""
    from graphical_gan_amd.models import Config, GraphicalGAN
    m = GraphicalGAN(Config('cifar10', batch_size=4, n_coms=5, mode='local_ep', mode_k=mode_k))
    feed = m.feed_buffers('cpu')
    assert ('gumbel_u' in feed) == (mode_k != ST)
    assert tuple(feed['k_onehot'].shape) == (4, 5)


def test_new_entry_points_are_exported_and_bound():
    import ctypes as C
    from graphical_gan_amd import _lib
    assert _lib.MODE_K == {'CONCRETE': 0, STC: 1, ST: 2}
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert 'GGAN_MODE_K_CONCRETE = 0, GGAN_MODE_K_STC = 1, GGAN_MODE_K_ST = 2' in hdr
    assert int(re.search(r'#define GGAN_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == 800
    for name in ('ggan_gmm_latent_st_fwd', 'ggan_gmm_latent_st_bwd'):
        assert name in _lib.SIGNATURES and re.search(r'\bint %s\(' % name, hdr), name
    L = _lib.load()
    fwd, bwd = L.ggan_gmm_latent_st_fwd, L.ggan_gmm_latent_st_bwd
    assert len(fwd.argtypes) == 13 and len(bwd.argtypes) == 13
    # argument checks answer before any device work: a mode that is not straight-through, missing pointers
    p = C.c_void_p(8)
    n = C.c_void_p(0)
    assert fwd(p, p, p, p, p, p, 2, 3, 4, 0.0, 0.1, 0, n) != 0 and 'straight-through' in L.ggan_last_error().decode()
    assert fwd(p, p, n, p, p, p, 2, 3, 4, 0.0, 0.1, 1, n) != 0                    # STC needs the Gumbel draws
    assert fwd(p, p, n, n, p, p, 2, 257, 4, 0.0, 0.1, 2, n) != 0                  # K <= 256
    assert bwd(p, p, n, p, p, p, p, 2, 3, 4, 0.1, 1, n) != 0                      # STC needs the soft assignment
    assert bwd(p, p, n, n, n, p, p, 2, 3, 4, 0.1, 2, n) != 0                      # no incoming gradient


def test_fixture_cases_margins_and_random_nodes():
    want = {('gmgan_inference_mnist', 'local_ep', STC), ('gmgan_inference_cifar10', 'local_epce', STC),
            ('gmgan_inference_cifar10', 'local_ep', ST), ('gmgan_inference_svhn', 'local_ep', ST)}
    assert {tuple(k.split(':')) for k in TRACE} >= want
    for key, t in TRACE.items():
        script, mode, mode_k = key.split(':')
        c = t['constants']
        assert (c['MODE'], c['MODE_K'], c['N_COMS'], c['BATCH_SIZE']) == (mode, mode_k, 5, 6) and t['mode_k'] == mode_k
        assert t['argmax_calls'] > 0 and t['argmax_margin'] >= t['margin_bound'] >= 1e-3, key
        B, K = c['BATCH_SIZE'], c['N_COMS']
        gumbel = [n for n in t['random_nodes'] if n[1] == 'uniform' and n[2] == [B, K]]
        if mode_k == ST:
            assert not gumbel, key                     # (no sample_gumbel in HyperExtractor under STRAIGHT_THROUGHT)
        else:
            assert gumbel, key
        ids = {n[0] for n in t['random_nodes']}
        runs = [r for r in t['runs'] if r['train']]
        assert len(runs) == 5 and all({d[0] for d in r['draws']} <= ids for r in runs)
        n = len(t['names'])
        assert t['names'] == sorted(t['names']) and len(t['shapes']) == len(t['first_grads']) == len(t['gmax']) == len(t['final']) == n
        assert all(len(d) == 2 + t['final_samples'] for d in t['final'])
        assert all(d is None or (len(d) == 10 and d[1] >= 0) for d in t['first_grads'])
        # the mixture means learn through the assignment in every mode, and the generator steps are in the trace
        assert t['gmax'][t['names'].index('Generator.Hyper.Mu')] > 0, key
        assert any(r['train'][0]['optimizer'] == 0 for r in runs), key
