"""not-gpu: the host side of the evaluation passes (graphical_gan_amd/evaluate.py) -- the reference's clustering-accuracy loop against
the decoding rule of ggan_cluster_accuracy, the new C entry points' declarations and bindings, and the driver's eval switches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_accuracy(prob_c, y):
    """gmgan_inference_mnist.py:513-529, literally (Python 3 spelling): the +1000 relabelling included"""
    ind_max_prob = np.argmax(prob_c, axis=0)
    labels_for_clusters = y[ind_max_prob]
    clusters = np.argmax(prob_c, axis=1)
    for i in range(labels_for_clusters.shape[0]):
        clusters[clusters == i] = labels_for_clusters[i] + 1000
    clusters = clusters - 1000
    return np.mean((clusters == y).astype(np.float32))


def _cases():
    rng = np.random.default_rng(3)
    out = []
    # plain random posteriors
    for N, K in ((50, 5), (130, 30), (64, 50)):
        logits = 3 * rng.standard_normal((N, K)).astype(np.float32)
        P = np.exp(logits - logits.max(1, keepdims=True))
        out.append((P / P.sum(1, keepdims=True), rng.integers(0, 10, size=N)))
    # saturated rows (p = 1.0 exactly): column ties resolved to the lowest row; an all-zero column; components that win no row
    N, K = 40, 6
    P = np.zeros((N, K), np.float32)
    P[np.arange(N), rng.integers(0, 3, size=N)] = 1.0           # columns 3..5 are all zero, nobody is assigned to them
    out.append((P, rng.integers(0, 10, size=N)))
    # duplicated rows: equal probabilities in every column
    base = rng.random((8, 7)).astype(np.float32)
    P = np.concatenate([base, base, base[::-1]])
    P /= P.sum(1, keepdims=True)
    out.append((P.astype(np.float32), rng.integers(0, 4, size=len(P))))
    # row ties: two equal maxima within a row (first index wins)
    P = np.full((10, 4), 0.1, np.float32)
    P[:, 1] = P[:, 2] = 0.35
    out.append((P, np.arange(10) % 3))
    return out


@pytest.mark.parametrize('case', range(6))
def test_reference_accuracy_loop_equals_the_documented_decoding(case):
    from graphical_gan_amd import evaluate as E
    P, y = _cases()[case]
    N, K = P.shape
    ref = _reference_accuracy(P.copy(), y.copy())
    assert E.host_cluster_accuracy(P, y) == ref
    # the device rule: keys (p bits << 32 | 0xFFFFFFFF - row), column max, decode, count
    keys = E.column_keys(P)
    rows = (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    assert (rows == np.argmax(P, axis=0)).all()                 # lowest row on a tie, row 0 for an all-zero column
    correct = E.decode_cluster_accuracy(np.argmax(P, axis=1), y, keys)
    assert np.float32(correct / float(N)) == ref
    if case == 3:
        assert (rows[3:] == 0).all() and ref > 0


def test_relabelling_collision_matches_reference():
    """the +1000 trick relabels cluster i AFTER clusters 0..i-1 took labels; with fewer than 1000 components a label + 1000 never equals
    a later cluster index, so the reference's loop is the plain propagation -- also when a label equals a cluster index"""
    from graphical_gan_amd import evaluate as E
    P = np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1, 2]]
    y = np.array([1, 2, 0, 1, 2, 1])
    assert E.host_cluster_accuracy(P, y) == _reference_accuracy(P.copy(), y.copy()) == np.float32(5 / 6.)
    assert E.decode_cluster_accuracy(np.argmax(P, 1), y, E.column_keys(P)) == 5


def test_posterior_entry_points_declared_and_bound():
    from graphical_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    for name in ('ggan_gmm_posterior_assign', 'ggan_cluster_accuracy'):
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert int(re.search(r'#define GGAN_POSTERIOR_MAX_K (\d+)', hdr).group(1)) == _lib.POSTERIOR_MAX_K
    assert len(_lib.SIGNATURES['ggan_gmm_posterior_assign'][1]) == 11
    assert len(_lib.SIGNATURES['ggan_cluster_accuracy'][1]) == 7
    from graphical_gan_amd import functional as F
    assert callable(F.gmm_posterior_assign_) and callable(F.cluster_accuracy_)


def test_settings_without_eval_keys_take_no_eval_path():
    from graphical_gan_amd import run
    names = ['gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_mnist', 'gan_inference_face', 'gmgan_inference_cifar10',
             'gmgan_inference_svhn', 'gmgan_inference_mnist', 'gmgan_inference_face']
    for n in names:
        S = run.reference_block(n)
        assert not any(k in S for k in run.EVAL_KEYS), n
        assert run.eval_plan(S) is None
    assert run.eval_plan(dict(DATASET='mnist', BATCH_SIZE=8, ITERS=5, LOG_EVERY=2)) is None
    assert all(run.eval_due(None, it) == [] for it in range(300))


def test_eval_cadence_is_the_references(monkeypatch):
    from graphical_gan_amd import run
    for k in run.EVAL_KEYS:
        monkeypatch.delenv('GGAN_' + k, raising=False)
    S = run.eval_settings('/x/scripts/gmgan_inference_mnist.py')
    assert (S['DEV_EVERY'], S['SAMPLE_EVERY'], S['ACCURACY_EVERY']) == (100, 5000, 5000)
    assert 'ACCURACY_EVERY' not in run.eval_settings('gmgan_inference_cifar10')      # (as the reference: mnist only)
    plan = run.eval_plan(S)
    fired = {k: [it for it in range(10000) if k in run.eval_due(plan, it)] for k in plan}
    assert fired['DEV_EVERY'][:3] == [99, 199, 299] and len(fired['DEV_EVERY']) == 100
    assert fired['ACCURACY_EVERY'] == [4999, 9999] == fired['SAMPLE_EVERY']
    monkeypatch.setenv('GGAN_DEV_EVERY', '7')
    assert run.eval_settings('gan_inference_mnist')['DEV_EVERY'] == 7
    for name in os.listdir(os.path.join(ROOT, 'scripts')):
        if name.startswith(('gan_inference_', 'gmgan_inference_')):
            assert 'run.eval_settings(__file__)' in open(os.path.join(ROOT, 'scripts', name)).read(), name
