"""The driver loop shared by the counterpart scripts in scripts/ (same file names and UPPERCASE hyper-parameter blocks as the
reference's gan_inference_* / gmgan_inference_* / ssgan_inference_* scripts; their train loop is
gmgan_inference_cifar10.py:470-549: alternate one generator step and CRITIC_ITERS critic steps on fresh minibatches, log the
costs through tflib.plot, dump sample grids and a checkpoint every so often)."""
import contextlib
import functools
import itertools
import os
import time

import numpy as np
import torch

from . import checkpoint
from . import tflib as lib
from .data import DevicePrefetcher
from .engine import Trainer
from .evaluate import SET_SCORES, Evaluator, SequenceEvaluator
from .models_ssgan import StateSpaceGAN


def _batches(S, model, device):
    """real data through the py3 loaders.  A missing dataset raises, as the reference scripts do; the synthetic ring of the
    same shapes is an explicit opt-in (S['SYNTHETIC'] = True or GGAN_SYNTHETIC=1: smoke runs, benchmarks)."""
    ds = S['DATASET']
    synthetic_ok = bool(S.get('SYNTHETIC')) or os.environ.get('GGAN_SYNTHETIC', '') not in ('', '0')
    try:
        if synthetic_ok and S.get('SYNTHETIC') == 'force':
            raise FileNotFoundError('synthetic data requested')
        if ds == 'mnist':
            train, _, _ = lib.mnist.load(S['BATCH_SIZE'], S['BATCH_SIZE'])
            return DevicePrefetcher(train, device, pick=[0]), 'mnist.pkl.gz'
        if ds == 'cifar10':
            train, _ = lib.cifar10.load(S['BATCH_SIZE'], S.get('DATA_DIR', ''))
            return DevicePrefetcher(train, device, pick=[0], dtypes=[np.int32]), S.get('DATA_DIR')
        if ds == 'svhn':
            train, _ = lib.svhn.load(S['BATCH_SIZE'], S.get('DATA_DIR', ''))
            return DevicePrefetcher(train, device, pick=[0], dtypes=[np.int32]), S.get('DATA_DIR')
        if ds == 'face':
            train, _ = lib.celebA.load(S['BATCH_SIZE'], S.get('DATA_DIR', ''))
            return DevicePrefetcher(train, device, dtypes=[np.int32]), S.get('DATA_DIR')
        if ds == 'moving_mnist':
            train, _ = lib.simple_moving_mnist.load_video(S['LEN'], S['BATCH_SIZE'])

            def with_onehot():
                for x, y in train():
                    oh = np.zeros((len(y), S['N_C']), np.float32)
                    oh[np.arange(len(y)), y] = 1
                    yield x, oh
            return DevicePrefetcher(with_onehot, device), 'mnist.pkl.gz'
        if ds == 'chairs':
            train, _ = lib.chairs.load(S['LEN'], S['BATCH_SIZE'], 64, S.get('DATA_DIR', ''))
            return DevicePrefetcher(train, device), S.get('DATA_DIR')
    except FileNotFoundError as e:
        if not synthetic_ok:
            raise FileNotFoundError("%s -- dataset %r not found (DATA_DIR=%r); set S['SYNTHETIC'] = True or GGAN_SYNTHETIC=1 to "
                                    "train on synthetic minibatches instead" % (e, ds, S.get('DATA_DIR', '')))
        print('[run] %s -> synthetic minibatches (opt-in)' % e)
    ring = model.synthetic_ring(device, n=8)

    def forever():
        i = 0
        while True:
            yield ring[i % len(ring)]
            i += 1
    return forever(), 'synthetic'


# ---- the evaluation passes of the reference's driver loops (evaluate.py) ------------------------------------------------------------
EVAL_KEYS = ('DEV_EVERY', 'ACCURACY_EVERY', 'SAMPLE_EVERY')
SEQUENCE_DATASETS = ('moving_mnist', 'chairs')         # the state-space scripts: evaluate.SequenceEvaluator


def eval_plan(S):
    """{key: every} of the evaluation passes a settings block switches on, or None (the keys are absent by default: no pass runs)"""
    plan = {k: int(S[k]) for k in EVAL_KEYS if S.get(k)}
    return plan or None


def eval_due(plan, it):
    """the passes that fire after iteration `it`: it % N == N - 1, the reference's cadence (gmgan_inference_mnist.py:484,507,511)"""
    return [k for k, n in sorted((plan or {}).items()) if it % n == n - 1]


def eval_settings(script):
    """the cadence the reference's image script runs its passes at (dev costs every 100 iterations; samples / reconstructions every
    5000; the testing accuracy every 5000, gmgan_inference_mnist only), each overridable by $GGAN_<KEY> (e.g. GGAN_DEV_EVERY=10).
    The state-space scripts have only the video passes, every 5000 iterations (ssgan_inference_moving_mnist.py:673-677): SAMPLE_EVERY
    / $GGAN_SAMPLE_EVERY alone."""
    name = os.path.splitext(os.path.basename(script))[0]
    sequences = name in _SEQUENCE_SCRIPTS
    S = dict(SAMPLE_EVERY=5000, SCRIPT=name) if sequences else dict(DEV_EVERY=100, SAMPLE_EVERY=5000, SCRIPT=name)
    if name == 'gmgan_inference_mnist':
        S['ACCURACY_EVERY'] = 5000
    for k in (('SAMPLE_EVERY',) if sequences else EVAL_KEYS):
        if os.environ.get('GGAN_' + k):
            S[k] = int(os.environ['GGAN_' + k])
    return S


# the latent-space t-SNE pictures (evaluate.Evaluator.manifold) have a cadence of their own, outside EVAL_KEYS: every 50000 iterations in
# gan_inference_mnist.py:472, once after the last iteration in gmgan_inference_mnist.py:534, in no other script
MANIFOLD_KEYS = ('MANIFOLD_EVERY', 'MANIFOLD_AT_END')


def manifold_settings(script):
    """{'MANIFOLD_EVERY': 50000} for gan_inference_mnist, {'MANIFOLD_AT_END': True} for gmgan_inference_mnist, {} for every other script;
    $GGAN_MANIFOLD_EVERY sets (lowers) MANIFOLD_EVERY for those two"""
    name = os.path.splitext(os.path.basename(script))[0]
    S = {'gan_inference_mnist': {'MANIFOLD_EVERY': 50000}, 'gmgan_inference_mnist': {'MANIFOLD_AT_END': True}}.get(name, {})
    S = dict(S)
    k = 'MANIFOLD_EVERY'
    if S and os.environ.get('GGAN_' + k):
        S[k] = int(os.environ['GGAN_' + k])
    return S


def manifold_plan(S):
    """the MANIFOLD_* keys a settings block switches on, or None"""
    plan = {k: S[k] for k in MANIFOLD_KEYS if S.get(k)}
    return plan or None


def manifold_due(plan, it, iters):
    """does the pass fire after iteration `it` of `iters`: it % N == N - 1 (gan_inference_mnist.py:472), it == ITERS - 1 (gmgan :534)"""
    if not plan:
        return False
    n = int(plan.get('MANIFOLD_EVERY') or 0)
    return bool((n and it % n == n - 1) or (plan.get('MANIFOLD_AT_END') and it == iters - 1))


# the set-level dev scores (the rows of evaluate.SET_SCORES: dev mmd, dev precision / recall / density / coverage, dev knn accuracy, dev
# parzen ll, dev rec mse / psnr / ssim) are no pass of the reference's loops: each is off unless asked for, with a switch and a cadence of
# its own outside EVAL_KEYS
def score_settings(script):
    """{'<NAME>_EVERY': N} for every row of evaluate.SET_SCORES whose $GGAN_<NAME>_EVERY = N is set and which the script has: the eight
    image scripts have every row, the two state-space scripts those with `sequences` (dev rec alone: they have no single code or set of
    images to compare), any other name none"""
    name = os.path.splitext(os.path.basename(script))[0]
    if name not in _IMAGE_SCRIPTS and name not in _SEQUENCE_SCRIPTS:
        return {}
    rows = [r for r in SET_SCORES if name in _IMAGE_SCRIPTS or r.sequences is True]
    return {r.every: int(os.environ['GGAN_' + r.every]) for r in rows if os.environ.get('GGAN_' + r.every)}


def scores_due(S, it):
    """the names of the rows of evaluate.SET_SCORES that fire after iteration `it`, in the table's order: it % N == N - 1, the cadence of the
    other passes"""
    every = ((r.name, int(S.get(r.every) or 0)) for r in SET_SCORES)
    return tuple(name for name, n in every if n and it % n == n - 1)


# the least-squares linear probe of the codes (evaluate.Evaluator.probe_scores) is a pass of its own, outside the table of set-level scores:
# it needs the labelled TRAINING split as well and a fit step.  Off unless asked for
PROBE_DATA_SEED = 271828      # numpy's global RNG while the fit rows are drawn: the loaders' shuffle then gives the same rows every run


def probe_settings(script):
    """{'PROBE_EVERY': N} for the eight image scripts when $GGAN_PROBE_EVERY = N is set, {} otherwise and for every other script (the
    state-space scripts have no single code to probe); with $GGAN_PROBE_WIDE = 1 as well, {'PROBE_WIDE': True} too: the pass then also
    probes the pixels and the Extractor's top activations (evaluate.PROBE_WIDE_KEYS)"""
    name = os.path.splitext(os.path.basename(script))[0]
    n = os.environ.get('GGAN_PROBE_EVERY')
    out = {'PROBE_EVERY': int(n)} if n and name in _IMAGE_SCRIPTS else {}
    if name in _IMAGE_SCRIPTS and os.environ.get('GGAN_PROBE_WIDE') == '1':
        out['PROBE_WIDE'] = True
    return out


def probe_due(S, it):
    """does the probe pass fire after iteration `it`: it % N == N - 1, the cadence of the other passes"""
    n = int(S.get('PROBE_EVERY') or 0)
    return bool(n and it % n == n - 1)


def probe_sets(S):
    """the labelled minibatches the probe is fitted on: the leading PROBE_FIT_ROWS rows of the loader's TRAINING split (MNIST, CIFAR-10,
    SVHN), drawn with numpy's global RNG seeded to a constant -- the same rows every run -- inside the saved and restored state; None
    where the data have no labels (celebA, synthetic minibatches) or are not there.  The dev side is eval_sets' labelled dev set."""
    from .evaluate import PROBE_FIT_ROWS
    return _leading_training_rows(S, S.get('PROBE_FIT_ROWS', PROBE_FIT_ROWS))


def _leading_training_rows(S, rows, labels=True):
    """the leading `rows` rows of the loader's labelled TRAINING split as full minibatches [(images, labels)], drawn under PROBE_DATA_SEED
    inside the saved and restored numpy state; None without labels or data (probe_sets, classifier_sets).  labels=False (kmeans_sets):
    celebA's unlabelled training split will do too"""
    ds, B = S['DATASET'], S['BATCH_SIZE']
    n = max(1, int(rows) // B)
    state = np.random.get_state()
    try:
        if S.get('SYNTHETIC') == 'force' or ds not in (('mnist', 'cifar10', 'svhn') if labels else ('mnist', 'cifar10', 'svhn', 'face')):
            return None
        np.random.seed(PROBE_DATA_SEED)
        if ds == 'face':
            train = lib.celebA.load(B, S.get('DATA_DIR', ''))[0]
            return [(np.array(b[0] if isinstance(b, (tuple, list)) else b),) for b in itertools.islice(train(), n)] or None
        train = lib.mnist.load(B, B)[0] if ds == 'mnist' else getattr(lib, ds).load(B, S.get('DATA_DIR', ''))[0]
        fit = [tuple(np.array(a) for a in b[:2]) for b in itertools.islice(train(), n)]      # (copies: the loaders yield views of one array)
        return fit if labelled(fit) else None
    except FileNotFoundError:
        return None
    finally:
        np.random.set_state(state)


# the classifier score of generated images (evaluate.Evaluator.classifier_scores): the reference's inception-score pass under a classifier the
# run fits for itself on the labelled TRAINING split.  A pass of its own with a noise state of its own.  Off unless asked for
def classifier_settings(script):
    """{'CLS_EVERY': N} for the eight image scripts when $GGAN_CLS_EVERY = N is set, {} otherwise and for every other script (the state-space
    scripts have no single set of images to classify)"""
    name = os.path.splitext(os.path.basename(script))[0]
    n = os.environ.get('GGAN_CLS_EVERY')
    return {'CLS_EVERY': int(n)} if n and name in _IMAGE_SCRIPTS else {}


def classifier_due(S, it):
    """does the classifier pass fire after iteration `it`: it % N == N - 1, the cadence of the other passes"""
    n = int(S.get('CLS_EVERY') or 0)
    return bool(n and it % n == n - 1)


def classifier_sets(S):
    """the labelled minibatches the classifier is fitted on: the leading CLS_FIT_ROWS rows of the loader's TRAINING split, drawn as
    probe_sets draws its rows (the same constant seed: the probe's rows lead them); None where the data have no labels (celebA, synthetic
    minibatches) or are not there.  The dev side is eval_sets' labelled dev set."""
    from .evaluate import CLS_FIT_ROWS
    return _leading_training_rows(S, S.get('CLS_FIT_ROWS', CLS_FIT_ROWS))


# NDB of the generated images and the k-means clustering scores of the codes (evaluate.Evaluator.kmeans_scores): k-means fitted on the
# device, on the leading training rows (the bins) and on q_z of the dev set.  A pass of its own with a noise state of its own; no labels
# needed for the bins.  Off unless asked for
def kmeans_settings(script):
    """{'KMEANS_EVERY': N} for the eight image scripts when $GGAN_KMEANS_EVERY = N is set, {} otherwise and for every other script (the
    state-space scripts have no single set of images to bin)"""
    name = os.path.splitext(os.path.basename(script))[0]
    n = os.environ.get('GGAN_KMEANS_EVERY')
    return {'KMEANS_EVERY': int(n)} if n and name in _IMAGE_SCRIPTS else {}


def kmeans_due(S, it):
    """does the k-means pass fire after iteration `it`: it % N == N - 1, the cadence of the other passes"""
    n = int(S.get('KMEANS_EVERY') or 0)
    return bool(n and it % n == n - 1)


def kmeans_sets(S, model=None, device=None):
    """the minibatches the bins are fitted on: the leading KM_FIT_ROWS rows of the loader's TRAINING split, drawn as probe_sets draws its
    rows (the same constant seed: the probe's and the classifier's rows lead them), labels or not; without the dataset (synthetic
    minibatches) and with a model, a synthetic set of the training ring's shapes under a seed of its own; else None"""
    from .evaluate import KM_FIT_ROWS
    rows = S.get('KM_FIT_ROWS', KM_FIT_ROWS)
    fit = _leading_training_rows(S, rows, labels=False)
    if fit is None and model is not None and S['DATASET'] not in SEQUENCE_DATASETS:
        fit = [t for t in model.synthetic_ring(device, n=max(1, min(int(rows) // S['BATCH_SIZE'], 64)), seed=8765)]
    return fit


# the Frechet distance of codes and of projected images (evaluate.Evaluator.frechet_scores) is a pass of its own too: it draws its noise from
# a state of its own, so that switching it on moves no other logged number.  Off unless asked for
def frechet_settings(script):
    """{'FRECHET_EVERY': N} for the eight image scripts when $GGAN_FRECHET_EVERY = N is set, {} otherwise and for every other script (the
    state-space scripts have no single code to compare)"""
    name = os.path.splitext(os.path.basename(script))[0]
    n = os.environ.get('GGAN_FRECHET_EVERY')
    return {'FRECHET_EVERY': int(n)} if n and name in _IMAGE_SCRIPTS else {}


def frechet_due(S, it):
    """does the Frechet pass fire after iteration `it`: it % N == N - 1, the cadence of the other passes"""
    n = int(S.get('FRECHET_EVERY') or 0)
    return bool(n and it % n == n - 1)


# the sliced Wasserstein distance of codes and of images in the full pixel space (evaluate.Evaluator.swd_scores): a pass of its own as well,
# with a noise state of its own.  Off unless asked for
def swd_settings(script):
    """{'SWD_EVERY': N} for the eight image scripts when $GGAN_SWD_EVERY = N is set, {} otherwise and for every other script (the state-space
    scripts have no single code to compare; a frames-in-pixel-space twin needs fresh-noise sequence sets)"""
    name = os.path.splitext(os.path.basename(script))[0]
    n = os.environ.get('GGAN_SWD_EVERY')
    return {'SWD_EVERY': int(n)} if n and name in _IMAGE_SCRIPTS else {}


def swd_due(S, it):
    """does the sliced-Wasserstein pass fire after iteration `it`: it % N == N - 1, the cadence of the other passes"""
    n = int(S.get('SWD_EVERY') or 0)
    return bool(n and it % n == n - 1)


# an exponential moving average of the generator-side weights (engine.Trainer's ema_decay), kept on the device inside the steps and used by
# the passes only: off unless asked for; which weights the passes score is a second switch
EMA_EVAL_MODES = ('live', 'ema', 'both')


def ema_settings(script):
    """{'EMA_DECAY': d, 'EMA_EVAL': 'live' | 'ema' | 'both'} for the ten scripts when $GGAN_EMA_DECAY = d, a float in [0, 1), is set
    ($GGAN_EMA_EVAL: which weights the evaluation passes score, default 'live'), {} otherwise.  $GGAN_EMA_EVAL without a decay is an
    error: there would be nothing to score."""
    name = os.path.splitext(os.path.basename(script))[0]
    decay, which = os.environ.get('GGAN_EMA_DECAY'), os.environ.get('GGAN_EMA_EVAL')
    if name not in _IMAGE_SCRIPTS and name not in _SEQUENCE_SCRIPTS:
        return {}
    if not decay:
        if which:
            raise ValueError('GGAN_EMA_EVAL=%r needs GGAN_EMA_DECAY: no average is kept without a decay' % which)
        return {}
    return ema_check({'EMA_DECAY': decay, 'EMA_EVAL': which or 'live'})


def ema_check(S):
    """the EMA_* keys of a settings block, validated -> {'EMA_DECAY': float, 'EMA_EVAL': mode}, or {} when the block has no EMA_DECAY"""
    decay, which = S.get('EMA_DECAY'), S.get('EMA_EVAL')
    if decay is None or decay == '':
        if which and which != 'live':
            raise ValueError('EMA_EVAL=%r needs EMA_DECAY: no average is kept without a decay' % (which,))
        return {}
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError('EMA_DECAY=%r: a float in [0, 1)' % (decay,))
    if not 0.0 <= d < 1.0:
        raise ValueError('EMA_DECAY=%r: a float in [0, 1)' % (decay,))
    which = which or 'live'
    if which not in EMA_EVAL_MODES:
        raise ValueError('EMA_EVAL=%r: one of %s' % (which, ' / '.join(EMA_EVAL_MODES)))
    return {'EMA_DECAY': d, 'EMA_EVAL': which}


def ema_passes(S):
    """the weights the due passes run on, in order: ('live',), ('ema',) or ('live', 'ema')"""
    which = ema_check(S).get('EMA_EVAL', 'live')
    return ('live', 'ema') if which == 'both' else (which,)


@contextlib.contextmanager
def _on_weights(ev, weights):
    """the evaluator's passes inside the block score `weights`; 'ema': ONE visit of the averaged weights for all of them"""
    was, ev.weights = ev.weights, weights
    try:
        with ev._visit():
            yield
    finally:
        ev.weights = was


def rec_sequences(S, model, device):
    """the dev minibatches the state-space scripts' reconstruction pass scores: the leading ones of the loader's dev split, as many as
    REC_MAX_ROWS frames take (at least one) -- eval_sets keeps the first alone, which is all the video passes use; without the dataset,
    eval_sets' synthetic ones"""
    from .evaluate import REC_MAX_ROWS
    ds, B = S['DATASET'], S['BATCH_SIZE']
    n = max(1, int(S.get('REC_MAX_ROWS', REC_MAX_ROWS)) // (B * S['LEN']))
    state = np.random.get_state()
    try:
        if S.get('SYNTHETIC') == 'force':
            raise FileNotFoundError('synthetic data requested')
        if ds == 'moving_mnist':
            _, dev = lib.simple_moving_mnist.load_video(S['LEN'], B)
        elif ds == 'chairs':
            _, dev = lib.chairs.load(S['LEN'], B, 64, S.get('DATA_DIR', ''))
        else:
            raise ValueError('%r is no sequence dataset' % ds)
        return list(itertools.islice(dev(), n))
    except FileNotFoundError:
        return eval_sets(S, model, device)[0][:n]
    finally:
        np.random.set_state(state)


def labelled(batches):
    """are these minibatches (images, labels) pairs"""
    return bool(batches) and all(isinstance(b, (tuple, list)) and len(b) > 1 and b[1] is not None for b in batches)


def eval_sets(S, model, device):
    """(dev minibatches, labelled test minibatches or None) for the evaluation passes: tflib.mnist.load's dev and test generators, the
    test split of the CIFAR-10 / SVHN loaders, celebA's dev split, the dev split of the moving-MNIST / chairs loaders (the FIRST
    minibatch only: the video passes use nothing else) -- or, without the dataset, a synthetic dev set of the training ring's
    shapes and no test set.  Host lists of one epoch each; numpy's global RNG state (which the loaders' shuffles consume) is restored."""
    ds, B = S['DATASET'], S['BATCH_SIZE']
    state = np.random.get_state()
    try:
        if S.get('SYNTHETIC') == 'force':
            raise FileNotFoundError('synthetic data requested')
        if ds == 'mnist':
            _, dev, test = lib.mnist.load(B, B)
            return list(dev()), list(test())
        if ds in ('cifar10', 'svhn'):
            _, dev = getattr(lib, ds).load(B, S.get('DATA_DIR', ''))
            dev = list(dev())
            return dev, dev
        if ds == 'face':
            _, dev = lib.celebA.load(B, S.get('DATA_DIR', ''))
            return list(dev()), None
        if ds == 'moving_mnist':
            _, dev = lib.simple_moving_mnist.load_video(S['LEN'], B)
            return [next(iter(dev()))], None
        if ds == 'chairs':
            _, dev = lib.chairs.load(S['LEN'], B, 64, S.get('DATA_DIR', ''))
            return [next(iter(dev()))], None
        raise ValueError('no evaluation passes for dataset %r' % ds)
    except FileNotFoundError:
        return [t for t in model.synthetic_ring(device, n=8, seed=4321)], None
    finally:
        np.random.set_state(state)


# ---- the reference scripts' UPPERCASE hyper-parameter blocks, as data ------------------------------------------------------------
# per script: what differs between the image scripts (gan_inference_cifar10.py:39-79, gan_inference_svhn.py:32-72,
# gan_inference_mnist.py:31-70, gan_inference_face.py:33-50, gmgan_inference_cifar10.py:39-87, gmgan_inference_svhn.py:33-81,
# gmgan_inference_mnist.py:32-80, gmgan_inference_face.py:35-54); the MODE-dependent constants are derived below as the scripts do
_IMAGE_SCRIPTS = {
    'gan_inference_cifar10': dict(DATASET='cifar10', MODE='ali', BATCH_SIZE=64, ITERS=200000, DIM=64, OUTPUT_DIM=3072, BN_FLAG=True, DR_RATE=.2),
    'gan_inference_svhn': dict(DATASET='svhn', MODE='ali', BATCH_SIZE=64, ITERS=200000, DIM=64, OUTPUT_DIM=3072, BN_FLAG=False, DR_RATE=.2),
    'gan_inference_mnist': dict(DATASET='mnist', MODE='ali', BATCH_SIZE=50, ITERS=200000, DIM=64, OUTPUT_DIM=784, BN_FLAG=True),
    'gan_inference_face': dict(DATASET='face', MODE='ali', BATCH_SIZE=128, ITERS=100000, DIM_G=32, DIM_D=32, OUTPUT_DIM=12288,
                               BN_FLAG=False, DECAY=False, BETA2=.999),
    'gmgan_inference_cifar10': dict(DATASET='cifar10', MODE='local_ep', BATCH_SIZE=64, ITERS=200000, DIM=64, OUTPUT_DIM=3072, BN_FLAG=True,
                                    N_COMS=30, DR_RATE=.2),
    'gmgan_inference_svhn': dict(DATASET='svhn', MODE='local_ep', BATCH_SIZE=64, ITERS=200000, DIM=64, OUTPUT_DIM=3072, BN_FLAG=False,
                                 N_COMS=50, DR_RATE=.2),
    'gmgan_inference_mnist': dict(DATASET='mnist', MODE='local_ep', BATCH_SIZE=50, ITERS=200000, DIM=64, OUTPUT_DIM=784, BN_FLAG=True,
                                  N_COMS=30),
    'gmgan_inference_face': dict(DATASET='face', MODE='local_ep', BATCH_SIZE=128, ITERS=100000, DIM_G=32, DIM_D=32, OUTPUT_DIM=12288,
                                 BN_FLAG=False, DECAY=False, BETA2=.999, N_COMS=100),
}
# ssgan_inference_moving_mnist.py:27-55 / ssgan_inference_chairs.py:28-57
_SEQUENCE_SCRIPTS = {
    'ssgan_inference_moving_mnist': dict(DATASET='moving_mnist', MODE='local_ep', POS_MODE='naive_mean_field', ALI_MODE='concat_x',
                                         OP_DYN_MODE='res', BN_FLAG=False, DIM_LATENT_G=128, DIM_LATENT_L=8, DIM=32, DIM_OP=256, LEN=16,
                                         OUTPUT_SHAPE=[1, 64, 64], N_C=10, LAMBDA=0.1, LR=1e-4, BATCH_SIZE=50, BETA1=.5, BETA2=.999,
                                         ITERS=100000, CRITIC_ITERS=1),
    'ssgan_inference_chairs': dict(DATASET='chairs', MODE='local_ep', POS_MODE='naive_mean_field', ALI_MODE='concat_x', OP_COM_MODE='concat',
                                   OP_DYN_MODE='res_w', BN_FLAG=False, BN_FLAG_OP=False, DIM_LATENT_G=128, DIM_LATENT_L=8, DIM=32,
                                   DIM_OP=256, LEN=31, OUTPUT_SHAPE=[3, 64, 64], N_C=0, LAMBDA=0.1, LR=1e-4, BATCH_SIZE=50, BETA1=.5,
                                   BETA2=.999, ITERS=40000, CRITIC_ITERS=1),
}
_NO_CRITIC = ('vegan-mmd', 'vegan-kl', 'vegan-ikl', 'vegan-jsd', 'vae')
_RECON = ('alice', 'alice-z', 'alice-x', 'vegan', 'vegan-wgan-gp', 'vegan-kl', 'vegan-ikl', 'vegan-jsd', 'vegan-mmd', 'local_epce')


def reference_block(script, **overrides):
    """-> dict: the UPPERCASE hyper-parameter block the reference script of that name builds for its MODE (`script`: a file name or
    path, e.g. __file__), with `overrides` (MODE, ITERS, N_COMS, BATCH_SIZE, ...) applied BEFORE the MODE-dependent constants are
    derived, as editing the script's top would."""
    name = os.path.splitext(os.path.basename(script))[0]
    if name in _SEQUENCE_SCRIPTS:
        S = dict(_SEQUENCE_SCRIPTS[name])
        S.update(overrides)
        S.setdefault('BN_FLAG_G', S['BN_FLAG']); S.setdefault('BN_FLAG_E', S['BN_FLAG']); S.setdefault('BN_FLAG_D', S['BN_FLAG'])
        S.setdefault('DIM_LATENT_T', S['DIM_LATENT_L'])
        S.setdefault('OUTPUT_DIM', int(np.prod(S['OUTPUT_SHAPE'])))
        S.setdefault('N_VIS', S['BATCH_SIZE'])
        return S
    S = dict(_IMAGE_SCRIPTS[name])
    S.update(overrides)
    mode, bn = S['MODE'], S.pop('BN_FLAG')
    if mode in ('vegan-kl', 'vegan-ikl', 'vegan-jsd'):          # gan_inference_cifar10.py:40-49
        S.setdefault('TYPE_Q', 'learn_std'); S.setdefault('TYPE_P', 'no_std'); S.setdefault('Z_SAMPLES', 100)
    elif mode == 'vae':
        S.setdefault('TYPE_Q', 'learn_std'); S.setdefault('TYPE_P', 'learn_std')
    else:
        S.setdefault('TYPE_Q', 'no_std'); S.setdefault('TYPE_P', 'no_std')
    S.setdefault('STD', .1)
    if mode in _RECON:
        S.setdefault('DISTANCE_X', 'l2')
    S.setdefault('CRITIC_ITERS', 0 if mode in _NO_CRITIC else (5 if mode in ('vegan', 'vegan-wgan-gp', 'wali', 'wali-gp') else 1))   # :54-59
    S.setdefault('LAMBDA', 1.)
    # (the wali objectives build their own optimizers: RMSProp 5e-5 / Adam 1e-4, tflib/objs/gan_inference.py:4,28)
    S.setdefault('LR', {'wali-gp': 1e-4, 'wali': 5e-5}.get(mode, 2e-4))
    S.setdefault('BETA1', .9 if mode == 'vae' else .5)
    thin = mode in ('vegan', 'vegan-wgan-gp', 'vegan-kl', 'vegan-jsd', 'vegan-ikl')      # :72-77
    S.setdefault('BN_FLAG', False if thin else bn)
    S.setdefault('DIM_LATENT', 8 if thin else 128)
    if 'N_COMS' in S:
        S.setdefault('N_VIS', S['N_COMS'] * 10)
        S.setdefault('MODE_K', 'CONCRETE')
        if S['MODE_K'] == 'REINFORCE':
            S.setdefault('CONTROL_VARIATE', .0)
        elif S['MODE_K'] in ('CONCRETE', 'STRAIGHT_THROUGHT_CONCRETE'):
            S.setdefault('TEMP_INIT', .1)
            S.setdefault('TEMP', S['TEMP_INIT'])
    else:
        S.setdefault('N_VIS', S['BATCH_SIZE'] * 2)
    return S


def config(S):
    """the model configuration a settings block describes (Config / SSConfig); constants this implementation fixes are checked,
    not silently ignored"""
    if S['DATASET'] in ('moving_mnist', 'chairs'):
        from .models_ssgan import SSConfig
        assert S.get('DIM_LATENT_T', S['DIM_LATENT_L']) == S['DIM_LATENT_L'] and S.get('BETA1', .5) == .5
        # BN_FLAG_G / _E / _D default to BN_FLAG, as the scripts derive them (:31-34); BN_FLAG_OP (chairs :37) is read by no net of
        # the reference, so it is accepted and has no effect
        bn = bool(S.get('BN_FLAG', False))
        return SSConfig(batch_size=S['BATCH_SIZE'], length=S['LEN'], dim=S['DIM'], dim_op=S['DIM_OP'], dim_g=S['DIM_LATENT_G'],
                        dim_l=S['DIM_LATENT_L'], n_c=S['N_C'], pos_mode=S['POS_MODE'], op_dyn_mode=S['OP_DYN_MODE'], lr=S['LR'],
                        channels=S['OUTPUT_SHAPE'][0], dataset=S['DATASET'], mode=S['MODE'], lamb=S['LAMBDA'], ali_mode=S['ALI_MODE'],
                        bn_g=S.get('BN_FLAG_G', bn), bn_e=S.get('BN_FLAG_E', bn), bn_d=S.get('BN_FLAG_D', bn))
    from .models import Config
    mode_k = S.get('MODE_K', 'CONCRETE')
    if mode_k == 'REINFORCE':
        raise NotImplementedError('MODE_K = %r: the score-function estimator is not built (DESIGN.md 0)' % mode_k)
    if mode_k not in ('CONCRETE', 'STRAIGHT_THROUGHT_CONCRETE', 'STRAIGHT_THROUGHT'):
        raise ValueError('MODE_K = %r is none of the reference\'s values' % mode_k)
    if mode_k != 'CONCRETE' and S['DATASET'] == 'face':
        # (gmgan_inference_face.py:52,100-104 hard-codes the CONCRETE branch: the script has no MODE_K switch)
        raise NotImplementedError('MODE_K = %r: gmgan_inference_face builds only the CONCRETE relaxation' % mode_k)
    if S['MODE'] == 'vae':
        raise NotImplementedError('MODE vae: the reference Generator returns no decoder statistics (DESIGN.md 8)')
    if S['DATASET'] == 'face' and S.get('N_COMS') and S['MODE'] not in ('ali', 'local_ep'):
        # (gmgan_inference_face.py:35,148,204,268-277: the script builds the local critics or the joint one and has objectives for
        #  ali and local_ep alone; every other MODE ends in its raise('NotImplementedError'))
        raise NotImplementedError('MODE = %r: gmgan_inference_face runs ali and local_ep only (gmgan_inference_face.py:268-277)' % S['MODE'])
    assert S.get('DISTANCE_X', 'l2') == 'l2' and S.get('LAMBDA', 1.) == 1. and S.get('BETA1', .5) == .5 and S.get('Z_SAMPLES', 100) == 100, S
    assert S.get('DIM_G', S.get('DIM')) == S.get('DIM_D', S.get('DIM')), 'one model width'
    return Config(S['DATASET'], batch_size=S['BATCH_SIZE'], n_coms=S.get('N_COMS', 0), mode=S['MODE'], dim=S.get('DIM', S.get('DIM_G')),
                  dim_latent=S['DIM_LATENT'], bn=S['BN_FLAG'], temp=S.get('TEMP', 0.1), lr=S['LR'], mode_k=mode_k)


def train(S, cfg, model=None, out_dir=None):
    """S: dict of the script's UPPERCASE settings (needs DATASET, BATCH_SIZE, ITERS; optional SAVE_EVERY, LOG_EVERY, SEED;
    EMA_DECAY keeps an average of the generator-side weights and EMA_EVAL = 'live' | 'ema' | 'both' says which weights the passes score)."""
    lib.print_model_settings_dict(S)
    device = lib.get_device()
    np.random.seed(S.get('SEED', 0))
    torch.manual_seed(S.get('SEED', 0))
    ema = ema_check(S)
    tr = Trainer(cfg, device=device, graph=S.get('HIP_GRAPH', True), model=model, sync_bn=S.get('SYNC_BN', False),
                 ema_decay=ema.get('EMA_DECAY'))
    passes = ema_passes(S)
    batches, source = _batches(S, tr.model, device)
    print('[run] data: %s' % source)
    out_dir = out_dir or S.get('OUT_DIR')
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'logfile.txt'), 'a') as f:
            f.write('data source: %s\n' % source)
    # `time` = seconds per iteration since the start, on the device clock (HIP events on the Trainer's stream)
    timed = device.type == 'cuda'
    t0 = time.time()
    if timed:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(device))
    lead = tr.world == 1 or torch.distributed.get_rank() == 0          # (replicas: rank 0 evaluates and logs)
    sequences = isinstance(tr.model, StateSpaceGAN)
    # the reference's passes, the latent-space pictures and the set-level scores share ONE evaluator and ONE eval_sets call per run, each
    # made when the first pass that is on needs it
    the_eval = functools.lru_cache(None)(lambda: (SequenceEvaluator if sequences else Evaluator)(tr, S))
    the_sets = functools.lru_cache(None)(lambda: eval_sets(S, tr.model, device))
    plan = eval_plan(S) if lead else None
    if plan and sequences and not out_dir:
        print('[run] video passes skipped: no OUT_DIR to write them to')
        plan = None
    if plan:
        the_eval().set_fixed_data(the_sets()[0][0])
        if 'ACCURACY_EVERY' in plan and (the_sets()[1] is None or not tr.cfg.K):
            print('[run] testing accuracy skipped: %s' % ('no mixture prior (N_COMS)' if not tr.cfg.K else 'no labelled test set (%s data)' % source))
            plan.pop('ACCURACY_EVERY')
    manifold = manifold_plan(S) if lead else None
    if manifold:
        if sequences or tr.cfg.dataset != 'mnist':
            why = 'a pass of the MNIST scripts only'
        elif not out_dir:
            why = 'no OUT_DIR to write the pictures to'
        else:
            why = None if labelled(the_sets()[0]) else 'no labelled dev set (%s data)' % source
        if why:
            print('[run] latent-space t-SNE skipped: %s' % why)
            manifold = None
    # the set-level scores that are on (the rows of evaluate.SET_SCORES with an <NAME>_EVERY).  The state-space scripts have dev rec alone,
    # through their own evaluator and on dev minibatches of their own
    on = set(r.name for r in SET_SCORES if S.get(r.every)) if lead else set()
    if on and sequences:
        if 'rec' in on:
            the_eval()
            rec_dev = rec_sequences(S, tr.model, device)
        skipped = [r.title for r in SET_SCORES if r.name in on and r.sequences is not True]
        if skipped:
            print('[run] %s skipped: the state-space models have no single code to compare' % ' and '.join(skipped))
        on &= {'rec'}
    elif on:
        the_eval()
        for r in SET_SCORES:
            if r.name in on and 'labels' in r.needs and not labelled(the_sets()[0]):
                print('[run] %s skipped: no labelled dev set (%s data)' % (r.title, source))
                on.discard(r.name)
    # the linear probe of the codes: the labelled training rows it is fitted on are loaded once per run, and only where the pass is on
    probe = bool(S.get('PROBE_EVERY')) and lead
    the_fit = functools.lru_cache(None)(lambda: probe_sets(S))
    if probe and sequences:
        print('[run] dev probe accuracy skipped: the state-space models have no single code to compare')
        probe = False
    elif probe and not (labelled(the_sets()[0]) and the_fit()):
        print('[run] dev probe accuracy skipped: no labelled dev set and training split (%s data)' % source)
        probe = False
    # the Frechet distance of codes and of projected images: no labels needed, so every image script's data will do
    frechet = bool(S.get('FRECHET_EVERY')) and lead
    if frechet and sequences:
        print('[run] dev frechet skipped: the state-space models have no single code to compare')
        frechet = False
    # the sliced Wasserstein distance of codes and of images: no labels needed either
    swd = bool(S.get('SWD_EVERY')) and lead
    if swd and sequences:
        print('[run] dev swd skipped: the state-space models have no single code to compare')
        swd = False
    # the classifier score of generated images: the labelled training rows its classifier is fitted on are loaded once per run, where the pass is on
    cls = bool(S.get('CLS_EVERY')) and lead
    the_cls_fit = functools.lru_cache(None)(lambda: classifier_sets(S))
    if cls and sequences:
        print('[run] dev classifier score skipped: the state-space models have no single set of images to classify')
        cls = False
    elif cls and not (labelled(the_sets()[0]) and the_cls_fit()):
        print('[run] dev classifier score skipped: no labelled dev set and training split (%s data)' % source)
        cls = False
    # NDB and the k-means clustering scores: the training rows the bins are fitted on are loaded once per run, where the pass is on
    kmeans = bool(S.get('KMEANS_EVERY')) and lead
    the_km_fit = functools.lru_cache(None)(lambda: kmeans_sets(S, tr.model, device))
    if kmeans and sequences:
        print('[run] dev ndb skipped: the state-space models have no single set of images to bin')
        kmeans = False
    ev = the_eval() if plan or manifold or on or probe or frechet or swd or cls or kmeans else None
    ev_dev, ev_test = the_sets() if plan or manifold or probe or frechet or swd or cls or kmeans or (on and not sequences) else (None, None)
    flush = lambda: lib.plot.flush(out_dir, os.path.join(out_dir, 'logfile.txt') if out_dir else None)
    eval_ms = 0.0            # wall time of the evaluation passes (kept out of `time`)
    for it in range(S['ITERS']):
        if (it == 2 and isinstance(batches, DevicePrefetcher) and S.get('RING_FEED', True) and tr.graph_enabled
                and isinstance(tr.feed, dict) and 'real_x_int' in tr.feed and tr.world == 1):
            # int32 image data from a loader: from here on the host minibatches go into a device ring one iteration ahead and an
            # iteration is one graph replay (Trainer.use_host_ring); the loader's host iterator is continued where it stands
            tr.use_host_ring(batches)
        res = tr.iteration(it, batches)
        if it % S.get('LOG_EVERY', 100) == 0 or it == S['ITERS'] - 1:
            for k, v in res.items():
                lib.plot.plot(k.replace('_', ' '), float(v))
            if timed:
                ev1 = torch.cuda.Event(enable_timing=True)
                ev1.record(torch.cuda.current_stream(device))
                ev1.synchronize()
                lib.plot.plot('time', (ev0.elapsed_time(ev1) - eval_ms) * 1e-3 / (it + 1))
            else:
                lib.plot.plot('time', (time.time() - t0 - eval_ms * 1e-3) / (it + 1))
            flush()
        due = eval_due(plan, it)
        if due:
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _evaluate(ev, due, ev_dev, ev_test, it, out_dir, tr))
            flush()
        if manifold_due(manifold, it, S['ITERS']):
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: ev.manifold(ev_dev, out_dir, it))
        scores = dict.fromkeys((name for name in scores_due(S, it) if name in on), True)
        if scores:          # (one build of the sets for the image scores that are due; the sequences' frames for dev rec)
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.rec_scores(rec_dev) if sequences else ev.set_scores(ev_dev, **scores))))
            flush()
        if probe and probe_due(S, it):
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.probe_scores(the_fit(), ev_dev))))
            flush()
        if frechet and frechet_due(S, it):
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.frechet_scores(ev_dev))))
            flush()
        if swd and swd_due(S, it):
            for w in passes:
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.swd_scores(ev_dev))))
            flush()
        if cls and classifier_due(S, it):
            for w in passes:       # (the classifier is fitted by the first of these and scores both sets of weights)
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.classifier_scores(the_cls_fit(), ev_dev))))
            flush()
        if kmeans and kmeans_due(S, it):
            for w in passes:       # (the bins are fitted by the first of these and kept)
                with _on_weights(ev, w):
                    eval_ms += _timed(device, lambda: _plot(ev.tag(ev.kmeans_scores(the_km_fit(), ev_dev))))
            flush()
        lib.plot.tick()
        if out_dir and S.get('SAVE_EVERY') and (it + 1) % S['SAVE_EVERY'] == 0:
            checkpoint.save(os.path.join(out_dir, 'params_%d.npz' % (it + 1)), tr, data_source=source)
            _save_samples(tr, cfg, os.path.join(out_dir, 'samples_%d.png' % (it + 1)))
            if tr.has_ema():       # the same noise through the averaged Generator, beside it
                with tr.ema_weights():
                    _save_samples(tr, cfg, os.path.join(out_dir, 'samples_%d_ema.png' % (it + 1)))
    tr.flush()
    torch.cuda.synchronize()
    return tr


def _save_samples(tr, cfg, path):
    """the sample grid run.train writes with every checkpoint: the Generator on the noise of the last step, still in the Trainer's feed"""
    with torch.no_grad():
        nets = tr.model.forward_nets(tr.feed)
        # (the critic-free code-space modes never build Generator(p_z) in a step: samples are drawn here)
        fx = nets['fake_x'] if 'fake_x' in nets else tr.model.Generator(nets['p_z'])
    fx = fx.detach().float().cpu().numpy()
    side = getattr(cfg, 'S', 64)
    fx = fx.reshape(-1, getattr(cfg, 'C', 1), side, side)[:64]
    lo = 0.0 if getattr(cfg, 'out_act', 'tanh') == 'sigmoid' else -1.0
    lib.save_images.save_images(np.clip((fx - lo) / (1.0 - lo), 0, 1), path)


def _timed(device, fn):
    """fn() between two synchronisations of the device (the training work queued so far is not its time) -> milliseconds it took"""
    if device.type == 'cuda':
        torch.cuda.synchronize(device)
    t0 = time.time()
    fn()
    if device.type == 'cuda':
        torch.cuda.synchronize(device)
    return (time.time() - t0) * 1e3


def _plot(values):
    """a pass's {name: value} through lib.plot, in the pass's order"""
    for k, v in values.items():
        lib.plot.plot(k, v)


def _evaluate(ev, due, dev, test, it, out_dir, tr=None):
    """the passes due after iteration `it`, logged through lib.plot under the reference's names"""
    if 'DEV_EVERY' in due:
        _plot(ev.tag(ev.dev_costs(dev)))
    if 'ACCURACY_EVERY' in due:
        _plot(ev.tag({'testing accuracy': ev.cluster_accuracy(test)}))
    if 'SAMPLE_EVERY' in due and out_dir:
        if isinstance(ev, SequenceEvaluator):
            # generate_video(iteration, _data): the minibatch of the last critic step, still in the Trainer's feed buffer (read only)
            ev.save_videos(out_dir, it, train_data=tr.feed['real_x_unit'])
        else:
            ev.save_images(out_dir, it)
