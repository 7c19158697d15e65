"""gpu: the five set-level dev scores switched on together in run.train -- the names they log, in the order of evaluate.SET_SCORES, on the
live and then on the averaged weights -- and the one score the state-space scripts have of the five.  (Each score's values, its sets and
the untouched training are the subject of that score's own test file.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_mmd_sets_gpu as P  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ('MMD_EVERY', 'PRDC_EVERY', 'KNN_EVERY', 'PARZEN_EVERY', 'REC_EVERY')
REC = ['dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x']
KEYS = (['dev mmd z', 'dev mmd x']
        + ['dev %s %s' % (what, space) for space in ('z', 'x') for what in ('precision', 'recall', 'density', 'coverage')]
        + ['dev knn accuracy z', 'dev knn accuracy x'] + ['dev parzen ll x', 'dev parzen se x', 'dev parzen sigma x'] + REC)


def test_image_run_logs_the_nineteen_names_in_table_order_on_both_weights(gpu, tmp_path, monkeypatch):
    """labelled MNIST on disk, B = 8 and 24 dev rows: three minibatches, enough for Parzen's two and for PRDC_K = KNN_K = 5"""
    from graphical_gan_amd.models import Config
    assert len(KEYS) == 19 and len(set(KEYS)) == 19
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    S = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K,
             EMA_DECAY=0.5, EMA_EVAL='both', **dict.fromkeys(SWITCHES, 2))
    _, _, _, seen = P._train(S, Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16))
    dev = [(n, i, v) for n, i, v in seen if n.startswith('dev ')]
    both = KEYS + [k + ' ema' for k in KEYS]
    for it in (1, 3):
        assert [n for n, i, _ in dev if i == it] == both, it
    assert sorted(set(i for _, i, _ in dev)) == [1, 3]               # ... and no `dev ` name at any other iteration
    assert all(np.isfinite(v) for _, _, v in dev)


def test_sequence_run_has_dev_rec_alone_and_says_so_once(gpu, capsys):
    import test_ssgan_eval_gpu as SQ
    from graphical_gan_amd import run
    from graphical_gan_amd import tflib as lib
    S = dict(SQ._small('ssgan_inference_moving_mnist'), **dict.fromkeys(SWITCHES, 2))
    seen, orig, it0 = [], lib.plot.plot, lib.plot._iter[0]
    lib.plot.plot = lambda name, value: (seen.append((name, lib.plot._iter[0] - it0, float(value))), orig(name, value))[1]
    capsys.readouterr()
    try:
        SQ._train(S, run.config(S))
    finally:
        lib.plot.plot = orig
    dev = [(n, i, v) for n, i, v in seen if n.startswith('dev ')]
    for it in (1, 3, 5):
        assert [n for n, i, _ in dev if i == it] == REC, it
    assert sorted(set(i for _, i, _ in dev)) == [1, 3, 5] and all(np.isfinite(v) for _, _, v in dev)
    skipped = [line for line in capsys.readouterr().out.splitlines() if 'skipped' in line]
    assert skipped == ['[run] dev mmd and dev precision / recall / density / coverage and dev knn accuracy and dev parzen ll skipped: '
                       'the state-space models have no single code to compare']
