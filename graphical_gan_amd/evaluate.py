"""The observation passes of the reference's driver loops, forward only, on a Trainer's live parameters:

  dev_costs          `dev gen cost` (+ `dev rec cost` / `dev reg cost` where the MODE has a rec_penalty), averaged over the dev set
                     (gmgan_inference_mnist.py:484-504, gan_inference_cifar10.py:456-477);
  cluster_accuracy   `testing accuracy`: the unsupervised clustering accuracy of q_k_probs = softmax(q_k_logits) on the test set
                     (gmgan_inference_mnist.py:338,511-529) -- ggan_gmm_posterior_assign per minibatch, ggan_cluster_accuracy at the end;
  sample_grid        generate_image: Generator(HyperGenerator(tile(eye(N_COMS)), fixed noise)) with one column per component
                     (gmgan_inference_mnist.py:406-419), or Generator(fixed noise) with N_VIS = 2*BATCH_SIZE rows
                     (gan_inference_cifar10.py:370-378);
  reconstructions    reconstruct_image: real / Generator(Extractor(x)) pairs on a fixed dev minibatch (gmgan_inference_mnist.py:429-443);
  manifold           the latent-space pictures of the MNIST scripts (gan_inference_mnist.py:472-480, gmgan_inference_mnist.py:533-551):
                     q_z (and p_z, and the images) of the labelled dev set embedded by functional.tsne on the device, scattered by
                     tflib.visualization coloured by digit / mixture component / inferred component;
  mmd_scores         `dev mmd z` / `dev mmd x`: the unbiased mixture-of-RBF MMD^2 (tflib/objs/mmd.py:20-67, sigmas 2..80) between the aggregate
                     posterior q(z) and the prior p(z), and between the dev images and as many generated ones -- two set-level sums of
                     ggan_mix_rbf_sums.  Not a pass of the reference's loops: the stand-in for its inception score (README).
  prdc_scores        `dev precision|recall|density|coverage z|x`: k-NN-ball precision / recall (Kynkaanniemi et al. 2019) and density /
                     coverage (Naeem et al. 2020) of the same four sets -- ggan_knn_radii and ggan_ball_counts.  Not a pass of the
                     reference's loops either; it tells dropped modes from bad samples, which one MMD number cannot (README).
  knn_scores         `dev knn accuracy z|x`: the leave-one-out KNN_K-nearest-neighbour accuracy of the labelled dev set in code space
                     (q_z) and in pixel space -- ggan_knn_lists and ggan_knn_vote.  The one number that looks at a label: whether
                     images of one class are neighbours in z more often than in x (README).
  parzen_scores      `dev parzen ll x` / `dev parzen se x` / `dev parzen sigma x`: the Gaussian Parzen-window log-likelihood of held-out dev
                     images under a kernel density fitted to as many generated ones (Breuleux et al. 2011; Goodfellow et al. 2014),
                     pixels in [0, 1], the bandwidth chosen on the leading validation rows from PARZEN_SIGMAS -- ggan_parzen_lse, one
                     log-sum-exp sweep for all rows and bandwidths.  The one number with a published protocol (README for its limits).
  rec_scores         `dev rec mse x` / `dev rec psnr x` / `dev rec ssim x` / `dev rec ssim se x`: how well Generator(Extractor(x)) gives the dev
                     images back -- per-image mean squared error, PSNR and SSIM (Wang et al. 2004) in the unit pixel range, ggan_ssim_pairs.
                     The one pass that measures the round trip x -> q(z | x) -> Generator(z), and the one all ten scripts have:
                     SequenceEvaluator.rec_scores scores the state-space scripts' reconstructed sequences frame by frame.
  probe_scores       `dev probe accuracy z` / `fit probe accuracy z` / `dev probe accuracy xr`: a least-squares linear probe -- the closed-form
                     ridge classifier of functional.lsq_probe_fit on standardised columns -- fitted on q_z of labelled TRAINING rows and
                     scored on q_z of the labelled dev set, on its own fit rows, and (xr) the same probe on a fixed random projection of
                     the pixels to DIM_LATENT columns.  A pass of its own, not a row of SET_SCORES: it needs a second split and a fit
                     step, and draws its noise from a state of its own, so no other pass's values move.  Not a pass of the reference.
                     With PROBE_WIDE also PROBE_WIDE_KEYS: the same probe on the pixels (x) and on the Extractor's top activations (h),
                     up to 4096 columns (functional.lsq_probe_fit_wide), from the same forward pass.
  frechet_scores     `dev frechet z` / `dev frechet mean z` / `dev frechet xr` / `dev frechet mean xr`: the Frechet distance between Gaussians
                     fitted to two sets -- |dmu|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), the "FD" of FID, functional.frechet_distance -- of
                     q_z against as many prior draws (z) and of the dev images against as many generated ones, both through one fixed
                     random projection to FRECHET_PROJ_DIM columns (xr); the `mean` rows are the |dmu|^2 part.  A pass of its own with a
                     noise state of its own, no labels needed.  It stands in for tflib/inception_score.py, which needs a download; the
                     features are not Inception's, so no value is comparable with a published FID.
  swd_scores         `dev swd z` / `dev swd max z` / `dev swd x` / `dev swd max x`: the sliced Wasserstein distance -- both sets projected onto
                     SWD_DIRS fixed random unit directions, per direction W_p^p between the two sorted columns, the p-th root of the mean
                     over the directions and (`max`) of the largest, functional.sliced_wasserstein_projected -- of q_z against as many
                     prior draws (z) and of the dev images against as many generated ones in the FULL pixel space (x: 784 / 3072 / 12288
                     columns, pixels in [0, 1]).  No kernel width, no Gaussian fit, no column cap.  A pass of its own with a noise state
                     of its own, no labels needed.  It too stands in for tflib/inception_score.py; a Monte-Carlo estimate over the
                     drawn directions, in pixel space, so no value is comparable with a published SWD.
  classifier_scores  `dev classifier score x` / `dev classifier score std x` / `dev classifier score data` / `dev classifier accuracy` /
                     `dev classifier frechet x`: the reference's own sample pass (gan_inference_cifar10.py:381-391,483-487: 50000 images
                     from fresh prior noise, the inception-score formula of tflib/inception_score.py:47-53 over ten splits) under a
                     classifier the run fits for itself on labelled training rows (classifier.ImageClassifier, functional.SoftmaxXent)
                     in place of the downloaded Inception graph -- functional.class_score of its logits --, with the same score of the
                     dev images, its accuracy on them, and the Frechet distance of its 128-wide features.  A pass of its own with a
                     noise state of its own; labelled data only.  The name `inception score` is not logged: no value is comparable
                     with a published inception score or FID, nor with a value under another classifier ($GGAN_CLS_CKPT shares one).

The passes are safe in the middle of training: they run under torch.no_grad() on the current stream only (no second stream, no
collective), with a feed dict and a noise generator state of their own -- the Trainer's static feed buffers, ring slots and noise state
are never written -- and with numpy's global RNG state restored afterwards (the loaders' shuffles and the layers' initial-value draws
consume it; the training data order must not depend on whether evaluation is on).  BatchNorm uses the statistics of each evaluation
minibatch, as the reference's graph does (tflib/ops/batchnorm.py: the scripts pass no is_training).

The state-space scripts have no dev cost; their passes are pictures (ssgan_inference_moving_mnist.py:568-618, ssgan_inference_chairs.py:560-606),
run by SequenceEvaluator on a models_ssgan.StateSpaceGAN under the same rules:

  samples            generate_video: Generator(fixed_noise_g, DynamicGenerator(pre_fixed_noise), fixed_y), N_VIS = BATCH_SIZE sequences, a
                     fresh epsilon per call; written beside the last training minibatch (samples_<it>, train_data_<it>);
  reconstructions    reconstruct_video: rec_x = Generator(q_z_g, q_z_l, real_y) on a fixed dev minibatch (reconstruction_<it>);
  disentangle        dis_x = Generator(dis_g, q_z_l, dis_y): ONE global code for every sequence (and class 1 for moving-MNIST) with the
                     per-frame codes extracted from a fixed dev minibatch (disentangle_<it>).

Each is written as a .png sheet (one sequence per row) and a looping .gif; the bytes of both come from one ggan_video_sheet_u8 launch.

`python -m graphical_gan_amd.evaluate CKPT --script gmgan_inference_mnist [--data-dir DIR]` scores a saved checkpoint
(`--out-dir DIR --manifold` also writes the latent-space pictures of the two MNIST scripts, `--mmd` adds the two MMD^2 rows, `--prdc` the eight precision / recall / density / coverage rows, `--knn` the two k-NN accuracy rows, `--parzen` the three Parzen-window rows, `--rec` the four reconstruction rows, `--probe` the three linear-probe rows, `--frechet` the four Frechet-distance rows, `--swd` the four sliced-Wasserstein rows, `--cls` the five classifier-score rows, `--kmeans` the five NDB / k-means rows);
`... CKPT --script ssgan_inference_moving_mnist|ssgan_inference_chairs [--data-dir DIR] --out-dir DIR` writes the four pairs of files;
`--rec` prints the four reconstruction rows of the sequences' frames, and alone needs no --out-dir.

Every pass can look at an exponential moving average of the generator-side weights instead of the last iterate (engine.Trainer's
ema_decay; no part of the reference): an evaluator with `weights = 'ema'` runs its passes inside Trainer.ema_weights(), `tag` / `_fname`
give the names (' ema') and files ('_ema') of what it then reports, and `... CKPT --ema` scores the `ema/gen/` keys of a checkpoint.
The critic has no average: `dev gen cost ema` sets the averaged Generator / Extractor against the live critic."""
import argparse
import collections
import contextlib
import os
import time

import numpy as np
import torch

from . import functional as F
from . import tflib as lib

MMD_MAX_ROWS = 10000      # rows per set of the mmd_scores pass (settings: MMD_MAX_ROWS)
PRDC_MAX_ROWS = 10000     # rows per set of the prdc_scores pass (settings: PRDC_MAX_ROWS)
PRDC_K = 5                # neighbours of its k-NN balls (settings: PRDC_K; at most functional.PRDC_MAX_K)
KNN_MAX_ROWS = 10000      # rows of the knn_scores pass (settings: KNN_MAX_ROWS)
KNN_K = 5                 # neighbours that vote in it (settings: KNN_K; at most functional.KNN_MAX_K)
PARZEN_MAX_ROWS = 10000   # rows per set of the parzen_scores pass (settings: PARZEN_MAX_ROWS): the protocol's 10000 generated samples
PARZEN_VALID_ROWS = 1000  # leading dev rows its bandwidth is chosen on (settings: PARZEN_VALID_ROWS)
PARZEN_SIGMAS = np.logspace(-1, 0, 10)    # the protocol's bandwidth grid, in [0, 1] pixel units (settings: PARZEN_SIGMAS; at most functional.PARZEN_MAX_SIGMAS)
REC_MAX_ROWS = 10000      # rows (images; frames of the state-space scripts) of the rec_scores passes (settings: REC_MAX_ROWS)
PROBE_FIT_ROWS = 10000    # labelled training rows the probe_scores pass fits on (settings: PROBE_FIT_ROWS; may be raised to the whole split)
PROBE_MAX_ROWS = 10000    # labelled dev rows it scores (settings: PROBE_MAX_ROWS)
PROBE_RIDGE = 1e-2        # its ridge, on standardised features (settings: PROBE_RIDGE)
PROBE_SLAB_ROWS = 10000   # images it keeps on the device at a time: only the codes of a slab stay
PROBE_SEED = 104729       # offset of its own noise state, and of its projection matrix, from the evaluator's seed
PROBE_KEYS = ('dev probe accuracy z', 'fit probe accuracy z', 'dev probe accuracy xr')
PROBE_WIDE_KEYS = ('dev probe accuracy x', 'fit probe accuracy x', 'dev probe accuracy h', 'fit probe accuracy h')      # with PROBE_WIDE, after PROBE_KEYS
FRECHET_MAX_ROWS = 10000  # rows per set of the frechet_scores pass (settings: FRECHET_MAX_ROWS)
FRECHET_PROJ_DIM = 128    # columns of its fixed random projection of the pixels: functional.FRECHET_MAX_DIM, whatever DIM_LATENT is
FRECHET_SEED = 130003     # offset of its own noise state, and of its projection matrix, from the evaluator's seed
FRECHET_KEYS = ('dev frechet z', 'dev frechet mean z', 'dev frechet xr', 'dev frechet mean xr')
SWD_MAX_ROWS = 10000      # rows per set of the swd_scores pass (settings: SWD_MAX_ROWS)
SWD_DIRS = 512            # its random unit directions, drawn once per evaluator (settings: SWD_DIRS)
SWD_P = 2                 # its exponent, 1 or 2 (settings: SWD_P)
SWD_SEED = 155317         # offset of its own noise state, and of its direction matrices, from the evaluator's seed
SWD_KEYS = ('dev swd z', 'dev swd max z', 'dev swd x', 'dev swd max x')
CLS_SAMPLES = 50000       # generated rows the classifier_scores pass scores, floor(CLS_SAMPLES / B) minibatches: the reference's count (settings: CLS_SAMPLES)
CLS_MAX_ROWS = 10000      # labelled dev rows it scores (settings: CLS_MAX_ROWS)
CLS_SPLITS = 10           # splits of its score: the reference's (settings: CLS_SPLITS; at most functional.CLS_MAX_SPLITS)
CLS_FIT_ROWS = 20000      # labelled training rows its classifier is fitted on (settings: CLS_FIT_ROWS)
CLS_EPOCHS = 4            # passes over them (settings: CLS_EPOCHS)
CLS_SEED = 179426         # offset of its own noise state, and of the classifier's initial values, from the evaluator's seed
CLS_KEYS = ('dev classifier score x', 'dev classifier score std x', 'dev classifier score data', 'dev classifier accuracy', 'dev classifier frechet x')
KM_BINS = 100             # the bins of the kmeans_scores pass's NDB (settings: KM_BINS; at most functional.KMEANS_MAX_K)
KM_FIT_ROWS = 20000       # leading training rows its bins are fitted on (settings: KM_FIT_ROWS)
KM_SAMPLES = 20000        # generated rows it bins, floor(KM_SAMPLES / B) fresh-noise minibatches (settings: KM_SAMPLES)
KM_MAX_ROWS = 10000       # dev rows it bins and clusters (settings: KM_MAX_ROWS)
KM_ITERS = 50             # Lloyd iterations of either fit (settings: KM_ITERS)
KM_Z_THRESHOLD = 1.959963984540054    # the z statistic above which a bin differs: two-sided 5 % (settings: KM_Z_THRESHOLD)
KM_SEED = 193939          # offset of its own noise state, and of the uniforms of its seedings, from the evaluator's seed
KM_KEYS = ('dev ndb x', 'dev ndb js x', 'dev ndb data', 'dev kmeans accuracy z', 'dev kmeans nmi z')
EVAL_SEED = 7919          # offset of the evaluator's noise seeds from the settings seed (the Trainer's stream of draws is not touched)

# the reference's output file names, per script: (samples, reconstructions), formatted with frame= and mode=
_NAMES = {
    'gan_inference_mnist': ('{mode}_mnist_samples_{frame}.png', '{mode}_mnist_reconstruction_{frame}.png'),
    'gmgan_inference_cifar10': ('{frame}_samples_{mode}.png', '{mode}_reconstruction_{frame}.png'),
    'gmgan_inference_svhn': ('{frame}_samples_{mode}.png', '{mode}_reconstruction_{frame}.png'),
    'gmgan_inference_mnist': ('{frame}_samples_{mode}.png', '{frame}_reconstruction_{mode}.png'),
    'gmgan_inference_face': ('{frame}_samples_{mode}.png', '{frame}_reconstruction_{mode}.png'),
}
# the t-SNE scatters: (file name, point set, label set) -- gan_inference_mnist.py:480; gmgan_inference_mnist.py:546-551, whose `cluster` and
# `dev_data_vis` pictures are ONE embedding of the images
MANIFOLD_SCRIPTS = ('gan_inference_mnist', 'gmgan_inference_mnist')      # the two scripts of the reference that call TSNE()
_MANIFOLD = (('{mode}_mnist_manifold_{frame}.png', 'z', 'y'),)
_MANIFOLD_K = (('{frame}_manifold_{mode}.png', 'z', 'y'), ('{frame}_prior_{mode}.png', 'pz', 'pk'),
               ('{frame}_cluster_{mode}.png', 'x', 'qk'), ('{frame}_dev_data_vis_{mode}.png', 'x', 'y'))
_DEFAULT_NAMES = ('{mode}_samples_{frame}.png', '{mode}_reconstruction_{frame}.png')       # gan_inference_cifar10 / svhn / face
_DEFAULT_NAMES_K = _NAMES['gmgan_inference_cifar10']                                         # a mixture model of no named script


def host_cluster_accuracy(prob_c, y):
    """gmgan_inference_mnist.py:513-529 as the reference runs it (the +1000 relabelling included): prob_c [N, K], y [N] -> accuracy.
    (With more than 1000 components the relabelled values collide with later cluster indices and the loop relabels twice; every
    reference script has N_COMS <= 100.  ggan_cluster_accuracy propagates the labels directly.)"""
    prob_c, y = np.asarray(prob_c), np.asarray(y)
    ind_max_prob = np.argmax(prob_c, axis=0)
    labels_for_clusters = y[ind_max_prob]
    clusters = np.argmax(prob_c, axis=1)
    for i in range(labels_for_clusters.shape[0]):
        clusters[clusters == i] = labels_for_clusters[i] + 1000
    clusters = clusters - 1000
    return float(np.mean((clusters == y).astype(np.float32)))


def decode_cluster_accuracy(assign, labels, colbest):
    """the rule ggan_cluster_accuracy applies, on the host: the correct count from assign [N], labels [N] and the column keys colbest [K]
    (uint64: p bits << 32 | 0xFFFFFFFF - row)"""
    assign, labels = np.asarray(assign, np.int64), np.asarray(labels, np.int64)
    rows = 0xFFFFFFFF - (np.asarray(colbest).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    label_of = np.where(rows < len(labels), labels[np.minimum(rows, len(labels) - 1)], np.iinfo(np.int64).min)
    ok = (assign >= 0) & (assign < len(label_of))                    # (the kernel counts no match for an assignment outside [0, K))
    return int(np.sum(ok & (label_of[np.clip(assign, 0, len(label_of) - 1)] == labels)))


def column_keys(P):
    """the colbest keys of ggan_gmm_posterior_assign for fp32 probabilities P [N, K] (host restatement)"""
    P = np.ascontiguousarray(P, dtype=np.float32)
    bits = P.view(np.uint32).astype(np.uint64) << np.uint64(32)
    keys = bits | (np.uint64(0xFFFFFFFF) - np.arange(P.shape[0], dtype=np.uint64))[:, None]
    return keys.max(axis=0)


def _split(b):
    """a loader minibatch -> (images, labels or None)"""
    if isinstance(b, (tuple, list)):
        return b[0], (b[1] if len(b) > 1 else None)
    return b, None


REC_KEYS = ('dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x')


def _rec_stats(mse, ssim):
    """per-image device rows -> (float64 [4] device tensor: mean mse, mean of the per-image PSNR, mean SSIM, its standard error -- the
    population std / sqrt(count), as the Parzen pass --, the per-image PSNR rows)"""
    psnr, s = F.psnr_from_mse(mse), ssim.double()
    count = torch.full((), float(s.shape[0]), dtype=torch.float64, device=s.device)
    return torch.stack([mse.double().mean(), psnr.mean(), s.mean(), s.std(unbiased=False) / torch.sqrt(count)]), psnr


# ---- the set-level dev scores: one row each, in the order Evaluator.set_scores computes and logs them ---------------------------------
class SetScore(collections.namedtuple('SetScore', 'name needs title sequences help check score')):
    """name: the keyword of set_scores / evaluate_once, the flag --<name>, the settings key <NAME>_EVERY, $GGAN_<NAME>_EVERY and the row cap
    <NAME>_MAX_ROWS (default: the module constant of that name); needs: the sets _score_sets builds for it, of 'generated', 'labels', 'rec';
    title: what the 'skipped' messages call it; sequences: True where the state-space scripts have the score too, else why they have not;
    help: of the flag; check(ev, batches, cap): what is refused before any device work, or None; score(ev, sets, rows) -> (names, device
    tensors) from the leading `rows` rows, inside set_scores' guard"""
    __slots__ = ()
    every = property(lambda self: self.name.upper() + '_EVERY')

    def cap(self, S):
        key = self.name.upper() + '_MAX_ROWS'
        return int(S.get(key, globals()[key]))


_SPACES = (('z', 'z', 'pz'), ('x', 'x', 'gx'))         # (space, real set, generated set) of the two-sample scores


def _mmd_score(ev, sets, rows):
    if rows < 2:
        raise ValueError('the unbiased MMD needs at least 2 rows per set')
    return (['dev mmd ' + space for space, _, _ in _SPACES],
            [lib.objs.mmd.mix_rbf_mmd2(sets[a][:rows], sets[b][:rows], biased=False).double().reshape(1) for _, a, b in _SPACES])


def _prdc_score(ev, sets, rows):
    k = int(ev.S.get('PRDC_K', PRDC_K))
    if k > rows - 1:
        raise ValueError('PRDC_K = %d needs more than %d rows per set' % (k, rows))
    return (['dev %s %s' % (what, space) for space, _, _ in _SPACES for what in ('precision', 'recall', 'density', 'coverage')],
            [F.prdc(sets[a][:rows], sets[b][:rows], k) for _, a, b in _SPACES])


def _knn_check(ev, batches, cap):
    k = int(ev.S.get('KNN_K', KNN_K))
    if not 1 <= k <= F.KNN_MAX_K:
        raise ValueError('KNN_K = %d: 1 <= KNN_K <= %d expected' % (k, F.KNN_MAX_K))


def _knn_score(ev, sets, rows):
    k = int(ev.S.get('KNN_K', KNN_K))
    if k > rows - 1:
        raise ValueError('KNN_K = %d needs more than %d rows' % (k, rows))
    return (['dev knn accuracy ' + space for space in ('z', 'x')],
            [F.knn_accuracy(sets[space][:rows], sets['y'][:rows], k) for space in ('z', 'x')])


def _parzen_sigmas(S):
    return [float(v) for v in np.asarray(S.get('PARZEN_SIGMAS', PARZEN_SIGMAS), dtype=np.float64).reshape(-1)]


def _parzen_check(ev, batches, cap):
    B, sigmas = ev.cfg.B, _parzen_sigmas(ev.S)
    if not 1 <= len(sigmas) <= F.PARZEN_MAX_SIGMAS:
        raise ValueError('PARZEN_SIGMAS: 1 .. %d bandwidths expected, got %d' % (F.PARZEN_MAX_SIGMAS, len(sigmas)))
    full = sum(1 for b in batches if _split(b)[0].shape[0] == B)
    if min(full, max(1, cap // B)) < 2:
        raise ValueError('the Parzen pass needs at least 2 full minibatches of %d rows within PARZEN_MAX_ROWS = %d: one to '
                         'choose the bandwidth on, one to score' % (B, cap))


def _parzen_score(ev, sets, rows):
    return ['dev parzen ll x', 'dev parzen se x', 'dev parzen sigma x'], [ev._parzen(sets['x'][:rows], sets['gx'][:rows], _parzen_sigmas(ev.S))]


def _rec_score(ev, sets, rows):
    return list(REC_KEYS), [ev._rec(sets['x'][:rows], sets['rx'][:rows])]


_NO_CODE, _NO_IMAGES = 'the state-space scripts have no single code to compare', 'the state-space scripts have no single set of images to compare'
SET_SCORES = (
    SetScore('mmd', ('generated',), 'dev mmd', _NO_CODE,
             'also score the dev set by the unbiased MMD^2 of codes and of images (dev mmd z / dev mmd x; image scripts)', None, _mmd_score),
    SetScore('prdc', ('generated',), 'dev precision / recall / density / coverage', _NO_CODE,
             'also score the dev set by k-NN-ball precision / recall / density / coverage of codes and of images (eight dev rows; image scripts)',
             None, _prdc_score),
    SetScore('knn', ('labels',), 'dev knn accuracy', _NO_CODE,
             'also score the labelled dev set by the leave-one-out k-NN accuracy of codes and of images (dev knn accuracy z / x; image scripts)',
             _knn_check, _knn_score),
    SetScore('parzen', ('generated',), 'dev parzen ll', _NO_IMAGES,
             'also score the dev set by the Gaussian Parzen-window log-likelihood of held-out images under generated ones (dev parzen ll / se / '
             'sigma x; image scripts)', _parzen_check, _parzen_score),
    SetScore('rec', ('rec',), 'dev rec mse / psnr / ssim', True,
             'also score how well Generator(Extractor(x)) gives the dev set back: per-image (state-space scripts: per-frame) mse / PSNR / SSIM in '
             'the unit pixel range (dev rec mse / psnr / ssim / ssim se x; every script)', None, _rec_score),
)


def _known(where, scores):
    """the keywords of `scores` must be rows of SET_SCORES"""
    unknown = sorted(set(scores) - set(r.name for r in SET_SCORES))
    if unknown:
        raise TypeError('%s: no set-level score %s (known: %s)' % (where, ', '.join(unknown), ', '.join(r.name for r in SET_SCORES)))


class _Passes(object):
    """what the image and the sequence evaluator share: the guard every pass runs under, and which weights it looks at"""
    last_seconds = 0.0            # wall time of the last pass (device work included)
    weights = 'live'              # 'ema': every pass runs on the averaged generator-side weights (Trainer.ema_weights; the critic stays live)

    def tag(self, names):
        """the names a pass's values are logged under: {name: value} -> the same with ' ema' appended while weights == 'ema'"""
        return {k + ' ema': v for k, v in names.items()} if self.weights == 'ema' else names

    def _fname(self, path):
        """the file a pass writes: '_ema' in front of the extension while weights == 'ema'"""
        if self.weights != 'ema':
            return path
        stem, ext = os.path.splitext(path)
        return stem + '_ema' + ext

    @contextlib.contextmanager
    def _visit(self):
        """inside the block the parameters hold what `weights` names.  'live': nothing to do.  'ema': Trainer.ema_weights() (entering it
        again inside is free), except where the parameters already hold the average -- a Trainer whose weights ARE averaged ones read
        from a checkpoint (main --ema), or an averaging Trainer before its first generator step, whose average still is the weights"""
        if self.weights not in ('live', 'ema'):
            raise ValueError("weights: 'live' or 'ema', not %r" % (self.weights,))
        if self.weights == 'live' or self.tr.ema_loaded or self.tr.ema_pending():
            yield
        else:
            with self.tr.ema_weights():
                yield

    @contextlib.contextmanager
    def _guard(self):
        """a pass: on the weights `weights` names (_visit), no tape, the current stream only, the model's step-building state and numpy's
        RNG state as they were"""
        np_state = np.random.get_state()
        t0 = time.time()
        try:
            with self._visit(), torch.no_grad(), self.model.single_stream():
                yield
        finally:
            np.random.set_state(np_state)
            self.last_seconds = time.time() - t0


class Evaluator(_Passes):
    def __init__(self, trainer, settings, keep_noise=False):
        """trainer: an engine.Trainer of an image script (models.GraphicalGAN); settings: the script's UPPERCASE block (BATCH_SIZE, MODE,
        N_VIS, N_COMS, SEED).  keep_noise (tests): dev_costs keeps the noise it drew per batch in self.kept."""
        self.tr, self.S = trainer, settings
        self.model, self.cfg, self.device = trainer.model, trainer.cfg, trainer.device
        c = self.cfg
        seed = int(settings.get('SEED', 0)) + EVAL_SEED
        self.feed = self.model.feed_buffers(self.device)
        self.feed['rng_state'] = F.noise_state(self.device, seed)
        # fixed grid noise, drawn once from the settings seed (gmgan_inference_mnist.py:406-407, gan_inference_cifar10.py:371)
        n_vis = int(settings.get('N_VIS', (c.K * 10) if c.K else 2 * c.B))
        rng = np.random.RandomState(seed)
        self.fixed_noise = torch.as_tensor(rng.normal(size=(n_vis, c.dim_latent)).astype(np.float32)).to(self.device)
        self.fixed_k = None
        if c.K:
            assert n_vis % c.K == 0, 'N_VIS must be a multiple of N_COMS (gmgan_inference_mnist.py:80)'
            self.fixed_k = torch.as_tensor(np.tile(np.eye(c.K, dtype=np.float32), (n_vis // c.K, 1))).to(self.device)
        self.keep_noise, self.kept = keep_noise, []
        self.fixed_data = None            # the reconstruction minibatch (host), set_fixed_data / the first dev minibatch
        self.last_seconds = 0.0           # wall time of the last pass (device work included)

    # ---- plumbing ------------------------------------------------------------------------------------------------------------------
    def _stage(self, batches, want_labels=False):
        """minibatches (host arrays or device tensors, optionally (images, labels) tuples) -> (device [n, B, D] in the placeholder's
        dtype, device int32 labels [n*B] or None).  One upload per pass; a trailing partial minibatch is dropped, as the loaders do."""
        c = self.cfg
        xs, ys = [], []
        for b in batches:
            x, y = _split(b)
            if x.shape[0] != c.B:
                continue
            xs.append(x)
            ys.append(y)
        if not xs:
            raise ValueError('no full minibatch of %d rows to evaluate on' % c.B)
        dt = torch.float32 if c.dataset == 'mnist' else torch.int32
        if all(torch.is_tensor(x) for x in xs):
            X = torch.stack([x.to(self.device, dt).reshape(c.B, -1) for x in xs])
        else:
            X = torch.as_tensor(np.stack([np.asarray(x).reshape(c.B, -1) for x in xs]).astype(np.float32 if c.dataset == 'mnist' else np.int32))
            X = X.to(self.device)
        Y = None
        if want_labels:
            if any(y is None for y in ys):
                raise ValueError('cluster accuracy needs labelled minibatches')
            Y = torch.as_tensor(np.concatenate([np.asarray(y).reshape(-1) for y in ys]).astype(np.int32)).to(self.device)
        return X, Y

    def _load(self, x):
        self.model.set_batch(self.feed, x)
        self.model.sample_noise(self.feed)
        if self.keep_noise:
            self.kept.append({k: v.detach().cpu().numpy().copy() for k, v in self.feed.items()
                              if torch.is_tensor(v) and k != 'rng_state' and k not in ('x_pair', 'z_pair', 'k_pair')})

    # ---- the passes ----------------------------------------------------------------------------------------------------------------
    def dev_costs(self, batches):
        """mean over the dev minibatches of gen_cost, and of rec_penalty and gen_cost - rec_penalty where the MODE has one ->
        {'dev gen cost': .., 'dev rec cost': .., 'dev reg cost': ..}.  One host synchronisation per pass."""
        with self._guard():
            X, _ = self._stage(batches)
            n = X.shape[0]
            vals = torch.zeros((n, 2), dtype=torch.float32, device=self.device)
            has_rec = False
            self.kept = []
            for i in range(n):
                self._load(X[i])
                out = self.model.forward(self.feed, 'gen')
                vals[i, 0].copy_(out['gen_cost'].reshape(()))
                rec = out.get('rec_penalty')
                if rec is not None:
                    has_rec = True
                    vals[i, 1].copy_(rec.reshape(()))
            assert not F.pending_costs(), 'an evaluation cost was left owing its value'
            v = vals.cpu().numpy()
        res = {'dev gen cost': float(np.mean(v[:, 0]))}
        if has_rec:             # (gmgan_inference_mnist.py:488-496: per batch, in float32, as session.run returns them)
            res['dev rec cost'] = float(np.mean(v[:, 1]))
            res['dev reg cost'] = float(np.mean(v[:, 0] - v[:, 1]))
        return res

    def cluster_accuracy(self, batches, return_probs=False):
        """testing accuracy on labelled minibatches -> float, or (float, probs [N, K] numpy) with return_probs"""
        c = self.cfg
        if not c.K:
            raise ValueError('cluster accuracy needs a mixture prior (N_COMS)')
        with self._guard():
            X, Y = self._stage(batches, want_labels=True)
            n, B = X.shape[0], c.B
            N = n * B
            assign = torch.empty((N,), dtype=torch.int32, device=self.device)
            colbest = torch.zeros((c.K,), dtype=torch.int64, device=self.device)
            correct = torch.zeros((1,), dtype=torch.int32, device=self.device)
            probs = torch.empty((N, c.K), dtype=torch.float32, device=self.device) if return_probs else None
            log_pi = float(np.log(np.float32(1.0) / np.float32(c.K)))          # (as HyperExtractor)
            mu = self.model._mu()
            for i in range(n):
                self._load(X[i])
                q_z = self.model.Extractor(self.model.real_x(self.feed))
                F.gmm_posterior_assign_(q_z, mu, log_pi, i * B, assign, colbest, probs[i * B:(i + 1) * B] if probs is not None else None)
            F.cluster_accuracy_(assign, Y, colbest, correct)
            acc = int(correct.item()) / float(N)
            if return_probs:
                self.last_assign, self.last_colbest, self.last_labels = assign.cpu().numpy(), colbest.cpu().numpy(), Y.cpu().numpy()
                return acc, probs.cpu().numpy()
        return acc

    def latent_sets(self, batches):
        """the point sets of the latent-space pictures over the labelled minibatches, as device arrays: z = q_z [N, DIM_LATENT] and
        y = the labels (gan_inference_mnist.py:474-478); with a mixture prior also x = the images, pz = p_z of a fresh hyper_p_k /
        hyper_p_z per minibatch, pk = argmax hyper_p_k, qk = argmax q_k, q_k the sampled assignment of the configured MODE_K
        (gmgan_inference_mnist.py:535-543)"""
        c = self.cfg
        with self._guard():
            X, Y = self._stage(batches, want_labels=True)
            n, B = X.shape[0], c.B
            new = lambda w, dt=torch.float32: torch.empty((n * B, w) if w else (n * B,), dtype=dt, device=self.device)
            out = dict(z=new(c.dim_latent), y=Y)
            if c.K:
                out.update(x=new(c.output_dim), pz=new(c.dim_latent), pk=new(0, torch.int64), qk=new(0, torch.int64))
            self.kept = []
            for i in range(n):
                rows = slice(i * B, (i + 1) * B)
                self._load(X[i])
                real_x = self.model.real_x(self.feed)
                q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if c.agg else self.model.Extractor(real_x)
                q_z = q[0] if isinstance(q, tuple) else q
                out['z'][rows].copy_(q_z)
                if c.K:
                    out['x'][rows].copy_(real_x.float())
                    out['pz'][rows].copy_(self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']))
                    out['pk'][rows].copy_(torch.argmax(self.feed['k_onehot'], dim=1))
                    _, q_k = self.model.HyperExtractor(q_z, self.feed.get('gumbel_u'))
                    out['qk'][rows].copy_(torch.argmax(q_k, dim=1))
        return out

    def _score_sets(self, batches, rows, generated=True, labels=False, rec=False):
        """the four row sets the set-level scores compare, on the device, over the full minibatches and at most `rows` rows per set:
        z = q_z (the sampled code of the aggregated-posterior MODEs, as latent_sets), pz = as many fresh prior draws (through HyperGenerator
        with a mixture prior), x = real_x as the nets see it, gx = Generator(pz) minibatch by minibatch.  generated=False: z and x alone
        (the noise is drawn all the same: one stream of draws whichever sets are built).  labels: also y = the int32 labels of the same
        _stage call, row for row (labelled minibatches only).  rec: also rx = Generator(q_z) minibatch by minibatch -- the full minibatches
        reconstructions() runs, the Generator's BatchNorm on batch statistics; it draws no noise and moves no other set.  Called inside a
        pass's guard."""
        c = self.cfg
        X, Y = self._stage(batches, want_labels=labels)
        B = c.B
        n = min(X.shape[0], max(1, int(rows) // B))
        new = lambda w: torch.empty((n * B, w), dtype=torch.float32, device=self.device)
        sets = dict(z=new(c.dim_latent), x=new(c.output_dim))
        if generated:
            sets = dict(z=sets['z'], pz=new(c.dim_latent), x=sets['x'], gx=new(c.output_dim))
        if labels:
            sets['y'] = Y[:n * B]
        if rec:
            sets['rx'] = new(c.output_dim)
        self.kept = []
        for i in range(n):
            rows = slice(i * B, (i + 1) * B)
            self._load(X[i])
            real_x = self.model.real_x(self.feed)
            q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if c.agg else self.model.Extractor(real_x)
            q_z = q[0] if isinstance(q, tuple) else q
            sets['z'][rows].copy_(q_z)
            sets['x'][rows].copy_(real_x.float())
            if rec:
                sets['rx'][rows].copy_(self.model.Generator(q_z).float())
            if not generated:
                continue
            p_z = self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']) if c.K else self.feed['p_z_noise']
            sets['pz'][rows].copy_(p_z)
            sets['gx'][rows].copy_(self.model.Generator(sets['pz'][rows]).float())
        return sets

    def set_scores(self, batches, return_sets=False, **on):
        """the set-level scores asked for by keyword (the names of SET_SCORES: mmd=True, ...), from ONE build of the sets (_score_sets: one
        stream of noise draws, whichever scores are on) and ONE host synchronisation: mmd -> the two values of mmd_scores, prdc -> the eight
        of prdc_scores, knn -> the two of knn_scores, parzen -> the three of parzen_scores, rec -> the four of rec_scores, in the table's
        order.  With several on, each scores the leading rows its own row cap allows.  knn needs labelled minibatches (the labels come
        from the sets' own _stage call); parzen needs at least two full minibatches within its row cap (one to choose the bandwidth on, one
        to score) and at most functional.PARZEN_MAX_SIGMAS bandwidths; rec adds the set rx = Generator(q_z) and compares it with x image by
        image (its per-image rows stay in self.rec_rows).  The generated sets are built only where a score that is on needs them.
        return_sets: (values, {z, pz, x, gx}), with knn also y, with rec also rx, with knn alone {z, x, y}."""
        _known('set_scores', on)
        on = [r for r in SET_SCORES if on.get(r.name)]
        if not on:
            raise ValueError('set_scores: no score was asked for')
        B = self.cfg.B
        cap = {r.name: r.cap(self.S) for r in on}
        for r in on:
            if r.check:
                r.check(self, batches, cap[r.name])
        needs = set(n for r in on for n in r.needs)
        with self._guard():
            sets = self._score_sets(batches, max(cap.values()), generated='generated' in needs, labels='labels' in needs, rec='rec' in needs)
            names, vals = [], []
            for r in on:
                n, v = r.score(self, sets, min(sets['z'].shape[0], max(1, cap[r.name] // B) * B))
                names += n
                vals += v
            vals = torch.cat(vals).cpu().numpy()
        res = {name: float(v) for name, v in zip(names, vals)}
        return (res, sets) if return_sets else res

    def mmd_scores(self, batches, return_sets=False):
        """{'dev mmd z': unbiased MMD^2(q_z, p_z), 'dev mmd x': unbiased MMD^2(real_x, Generator(p_z))} over the full dev minibatches, at
        most MMD_MAX_ROWS rows per set (_score_sets).  The sets stay on the device; the two values come back in ONE host synchronisation.
        return_sets: (values, {z, pz, x, gx})."""
        return self.set_scores(batches, mmd=True, return_sets=return_sets)

    def prdc_scores(self, batches, return_sets=False):
        """{'dev precision z', 'dev recall z', 'dev density z', 'dev coverage z', and the same four with x}: precision / recall (Kynkaanniemi
        et al. 2019) and density / coverage (Naeem et al. 2020) from PRDC_K-NN balls (default 5) of the sets of mmd_scores -- real = q_z of
        the dev images / the dev images, generated = as many prior draws / Generator(p_z) -- at most PRDC_MAX_ROWS rows per set, by
        functional.prdc.  ONE host synchronisation for all eight.  return_sets: (values, {z, pz, x, gx})."""
        return self.set_scores(batches, prdc=True, return_sets=return_sets)

    def knn_scores(self, batches, return_sets=False):
        """{'dev knn accuracy z', 'dev knn accuracy x'}: the leave-one-out KNN_K-nearest-neighbour (default 5) accuracy of the labelled dev
        minibatches -- every row classified by the vote of its nearest OTHER rows, a tied vote to the smallest label -- in code space
        (q_z as _score_sets builds it) and in pixel space (real_x as the nets see it), at most KNN_MAX_ROWS rows, by
        functional.knn_accuracy.  ONE host synchronisation for both.  Unlabelled minibatches raise ValueError.
        return_sets: (values, {z, x, y})."""
        return self.set_scores(batches, knn=True, return_sets=return_sets)

    def _parzen(self, x, gx, sigmas):
        """(mean, standard error, bandwidth) of the Parzen-window log-likelihood of the held-out rows of x under the kernel density of gx
        -> float64 [3] device tensor.  ONE parzen_ll call over all rows and bandwidths; the leading v rows of x choose the bandwidth (the
        arg-max of their mean, the first on a tie), the rest are scored.  Selection and statistics stay on the device."""
        B, rows = self.cfg.B, x.shape[0]
        v = B * max(1, min(int(self.S.get('PARZEN_VALID_ROWS', PARZEN_VALID_ROWS)) // B, (rows // B) // 2))
        lo = 0.0 if self.cfg.out_act == 'sigmoid' else -1.0                 # (as _to_unit: the width of the pixel range is 1 - lo)
        ll = F.parzen_ll(x, gx, sigmas, scale=1.0 - lo)                       # [ns, rows] float64
        valid = ll[:, :v].mean(dim=1)
        # the first bandwidth whose validation mean is the largest (argmax alone does not promise which of equal values it returns)
        order = torch.arange(len(sigmas), device=ll.device)
        best = torch.where(valid == valid.max(), order, torch.full_like(order, len(sigmas))).min().reshape(1)
        held = ll[:, v:].index_select(0, best).reshape(-1)
        grid = torch.empty((len(sigmas),), dtype=torch.float64, device=ll.device)
        for g, sg in enumerate(sigmas):
            grid[g].fill_(sg)
        count = torch.full((), float(held.shape[0]), dtype=torch.float64, device=ll.device)
        return torch.stack([held.mean(), held.std(unbiased=False) / torch.sqrt(count), grid.index_select(0, best).reshape(())])

    def parzen_scores(self, batches, return_sets=False):
        """{'dev parzen ll x', 'dev parzen se x', 'dev parzen sigma x'}: the Gaussian Parzen-window log-likelihood (nats, pixels in [0, 1])
        of held-out dev images under a kernel density fitted to as many generated images (Breuleux et al. 2011; Goodfellow et al. 2014),
        over at most PARZEN_MAX_ROWS rows per set of _score_sets: the leading B max(1, min(PARZEN_VALID_ROWS // B, minibatches // 2)) dev
        rows choose the bandwidth from PARZEN_SIGMAS, the rest give the mean and its standard error (the population std / sqrt(count), as
        the protocol's script); sigma is the chosen bandwidth.  functional.parzen_ll, ONE host synchronisation for the three.  Fewer than
        two full minibatches raise ValueError.  There is no z twin: in code space the prior's density is known in closed form.  return_sets: (values, {z, pz, x, gx})."""
        return self.set_scores(batches, parzen=True, return_sets=return_sets)

    def _rec(self, x, rx):
        """the four reconstruction values of the rows of rx against those of x -> float64 [4] device tensor.  ONE ssim_pairs call over all
        rows, both sets in the range the nets see (the unit-scale map is in the kernel's formula); the per-image rows stay on the device in
        self.rec_rows = {mse, psnr, ssim}."""
        c = self.cfg
        unit = (1.0, 0.0) if c.out_act == 'sigmoid' else (0.5, 0.5)         # (as _to_unit)
        mse, ssim = F.ssim_pairs(rx, x, (c.C, c.S, c.S), unit)
        vals, psnr = _rec_stats(mse, ssim)
        self.rec_rows = dict(mse=mse, psnr=psnr, ssim=ssim)
        return vals

    def rec_scores(self, batches, return_rows=False):
        """{'dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x'}: how well the round trip Generator(Extractor(x)) gives
        the dev images back, image by image and with pixels in [0, 1] -- the mean squared error per image, the mean of the per-image PSNR in
        dB (-10 log10 max(mse, 1e-10)), the mean of the per-image SSIM (Wang et al. 2004: 11x11 Gaussian window, sigma 1.5, data range 1) and
        that mean's standard error -- over the full dev minibatches, at most REC_MAX_ROWS rows and at least one minibatch.  The
        reconstructions are those reconstructions() draws: Generator(q_z) a full minibatch at a time (with a stochastic Extractor the code is
        one sample).  functional.ssim_pairs, the statistics in float64 on the device, ONE host synchronisation for the four.
        return_rows: (values, {mse, psnr, ssim}: the per-image device rows)."""
        res = self.set_scores(batches, rec=True)
        return (res, self.rec_rows) if return_rows else res

    _probe_rng = _probe_matrix = None     # the probe pass's own noise state and projection matrix, made by its first call

    def _probe_projection(self):
        """the fixed random map of the pixels to DIM_LATENT columns: RandomState(seed).normal / sqrt(OUTPUT_DIM), drawn once per evaluator"""
        if self._probe_matrix is None:
            c = self.cfg
            rng = np.random.RandomState(int(self.S.get('SEED', 0)) + EVAL_SEED + PROBE_SEED)
            P = rng.normal(size=(c.output_dim, c.dim_latent)) / np.sqrt(float(c.output_dim))
            self._probe_matrix = torch.as_tensor(P.astype(np.float32)).to(self.device)
        return self._probe_matrix

    def _probe_codes(self, batches, rows, wide=()):
        """z = q_z (as _score_sets computes sets['z']), xr = real_x through _probe_projection and y = the int32 labels of the leading full
        minibatches, at most `rows` rows -> device tensors.  The images are staged PROBE_SLAB_ROWS rows at a time; only the codes stay.
        wide: which of 'x' (real_x flattened, in the scale the model reads) and 'h' (the Extractor's top activations) stay too, from the
        SAME forward pass -- 4 rows (OUTPUT_DIM + flat) bytes on the device until the pass returns."""
        c = self.cfg
        B = c.B
        full = [b for b in batches if _split(b)[0].shape[0] == B]
        if not full:
            raise ValueError('no full minibatch of %d rows to evaluate on' % B)
        n = min(len(full), max(1, int(rows) // B))
        if n * B > F.PROBE_MAX_ROWS:
            raise ValueError('the probe takes at most %d rows, got %d' % (F.PROBE_MAX_ROWS, n * B))
        new = lambda w: torch.empty((n * B, w), dtype=torch.float32, device=self.device)
        out = dict(z=new(c.dim_latent), xr=new(c.dim_latent), y=torch.empty((n * B,), dtype=torch.int32, device=self.device))
        out.update({k: new(c.output_dim if k == 'x' else c.flat) for k in wide})
        top = {'return_top': True} if 'h' in wide else {}
        per, proj = max(1, PROBE_SLAB_ROWS // B), self._probe_projection()
        for s0 in range(0, n, per):
            X, Y = self._stage(full[s0:min(n, s0 + per)], want_labels=True)
            out['y'][s0 * B:(s0 + X.shape[0]) * B].copy_(Y)
            for i in range(X.shape[0]):
                at = slice((s0 + i) * B, (s0 + i + 1) * B)
                self.model.set_batch(self.feed, X[i])
                self.model.sample_noise(self.feed)
                real_x = self.model.real_x(self.feed)
                q = self.model.Extractor(real_x, eps=self.feed['q_eps'], **top) if c.agg else self.model.Extractor(real_x, **top)
                if top:
                    q, h = q
                    out['h'][at].copy_(h)
                out['z'][at].copy_(q[0] if isinstance(q, tuple) else q)
                flat_x = real_x.float().reshape(B, -1).contiguous()
                out['xr'][at].copy_(F.Gemm.apply(flat_x, proj, None, False, False, F.ACT_NONE, 0.0))
                if 'x' in wide:
                    out['x'][at].copy_(flat_x)
        return out

    def probe_scores(self, fit_batches, dev_batches, return_fit=False, wide=False):
        """{'dev probe accuracy z', 'fit probe accuracy z', 'dev probe accuracy xr'}: a least-squares linear probe (functional.lsq_probe_fit:
        the ridge-regularised least-squares classifier on standardised columns, ridge PROBE_RIDGE, in closed form -- neither logistic
        regression nor an SVM) fitted on q_z of the leading PROBE_FIT_ROWS rows of the labelled TRAINING minibatches fit_batches and scored on
        q_z of the leading PROBE_MAX_ROWS rows of the labelled dev minibatches (dev), on its own fit rows (fit: a large gap to dev shows
        overfitting) and, as the baseline a code has to beat, the same probe on a fixed random projection of the pixels to DIM_LATENT
        columns (xr).  The code is the one _score_sets builds -- one sample with a stochastic Extractor --, so the value sits beside dev knn
        accuracy z.  The pass draws from a noise state of its own, swapped into the feed while it runs: every other pass logs the same values
        whether it is on or not.  ONE host synchronisation; a raised status word (a label out of range, a non-finite moment, a failed
        factorisation: a diverged model) gives nan and one printed message, no exception.
        return_fit: (values, {fit, fit_xr: the ProbeFit records, fit_z, fit_xr_rows, fit_y, dev_z, dev_xr, dev_y: the device rows}).
        wide (or the setting PROBE_WIDE): PROBE_WIDE_KEYS after the three -- the same classifier (functional.lsq_probe_fit_wide, ridge
        PROBE_WIDE_RIDGE, default PROBE_RIDGE) on the pixels x themselves, real_x flattened, and on h, the Extractor's top activations
        (the [B, flat] rows Extractor.Output reads), dev and fit each.  Both come from the forward pass that yields z: no second Extractor
        call, no further noise draw, and the three values above keep their bits.  The rows stay on the device for the pass: at the defaults
        up to 10000 x (3072 + 4096) x 4 bytes = 287 MB per split, plus 134 MB for a 4096-column fit.  A width above
        functional.WPROBE_MAX_DIM skips its pair with one message.  Still ONE host synchronisation.  return_fit gains fit_x, fit_h (the
        records) and fit_x_rows, fit_h_rows, dev_x, dev_h."""
        S = self.S
        ridge = float(S.get('PROBE_RIDGE', PROBE_RIDGE))
        if not ridge > 0.0:
            raise ValueError('PROBE_RIDGE = %s: a positive number expected' % ridge)
        wide = bool(wide or S.get('PROBE_WIDE'))
        wide_ridge = float(S.get('PROBE_WIDE_RIDGE', ridge))
        if wide and not wide_ridge > 0.0:
            raise ValueError('PROBE_WIDE_RIDGE = %s: a positive number expected' % wide_ridge)
        labels = [_split(b)[1] for b in list(fit_batches) + list(dev_batches)]
        if not fit_batches or not dev_batches or any(y is None for y in labels):
            raise ValueError('the probe needs labelled minibatches on both sides')
        classes = 1 + max(int(y.max()) for y in labels)             # (host labels: no device is asked)
        if not 1 <= classes <= F.PROBE_MAX_CLASSES:
            raise ValueError('the probe takes at most %d classes, got %d' % (F.PROBE_MAX_CLASSES, classes))
        with self._guard():
            if self._probe_rng is None:
                self._probe_rng = F.noise_state(self.device, int(S.get('SEED', 0)) + EVAL_SEED + PROBE_SEED)
            shared, self.feed['rng_state'] = self.feed['rng_state'], self._probe_rng
            sets = ()
            if wide:
                widths = dict(x=self.cfg.output_dim, h=self.cfg.flat)
                sets = tuple(k for k in ('x', 'h') if widths[k] <= F.WPROBE_MAX_DIM)
                for k in widths:
                    if k not in sets:
                        print('[evaluate] probe accuracy %s skipped: %d columns, the wide probe takes at most %d' % (k, widths[k], F.WPROBE_MAX_DIM))
            try:
                fit = self._probe_codes(fit_batches, S.get('PROBE_FIT_ROWS', PROBE_FIT_ROWS), sets)
                dev = self._probe_codes(dev_batches, S.get('PROBE_MAX_ROWS', PROBE_MAX_ROWS), sets)
            finally:
                self.feed['rng_state'] = shared
            pz = F.lsq_probe_fit(fit['z'], fit['y'], classes, ridge)
            px = F.lsq_probe_fit(fit['xr'], fit['y'], classes, ridge)
            hits = [F.lsq_probe_predict(pz, dev['z'], dev['y']), F.lsq_probe_predict(pz, fit['z'], fit['y']),
                    F.lsq_probe_predict(px, dev['xr'], dev['y'])]
            pw = {k: F.lsq_probe_fit_wide(fit[k], fit['y'], classes, wide_ridge) for k in sets}
            for k in sets:
                hits += [F.lsq_probe_predict_wide(pw[k], dev[k], dev['y']), F.lsq_probe_predict_wide(pw[k], fit[k], fit['y'])]
            host = torch.cat(hits + [pz.status, px.status] + [pw[k].status for k in sets]).cpu().numpy()
        nh = len(hits)
        rows = (dev['y'].shape[0], fit['y'].shape[0], dev['y'].shape[0]) + (dev['y'].shape[0], fit['y'].shape[0]) * len(sets)
        keys = PROBE_KEYS + tuple(k for k in PROBE_WIDE_KEYS if k[-1] in sets)
        status = (int(host[nh]), int(host[nh]), int(host[nh + 1])) + tuple(int(host[nh + 2 + i // 2]) for i in range(2 * len(sets)))
        if any(status):
            print('[evaluate] probe: status %d (z) / %d (xr)%s -- 1: a label out of range, 2: a non-finite moment or entry, 4: a pivot that is not '
                  'positive -- its values are nan' % (status[0], status[2], ''.join(' / %d (%s)' % (status[3 + 2 * i], k) for i, k in enumerate(sets))))
        res = {k: (float('nan') if st else int(h) / float(n)) for k, h, n, st in zip(keys, host[:nh], rows, status)}
        if return_fit:
            got = dict(fit=pz, fit_xr=px, fit_z=fit['z'], fit_xr_rows=fit['xr'], fit_y=fit['y'], dev_z=dev['z'], dev_xr=dev['xr'], dev_y=dev['y'])
            for k in sets:
                got.update({'fit_' + k: pw[k], 'fit_%s_rows' % k: fit[k], 'dev_' + k: dev[k]})
            return res, got
        return res

    _frechet_rng = _frechet_matrix = None     # the Frechet pass's own noise state and projection matrix, made by its first call

    def _frechet_projection(self):
        """the fixed random map of the pixels to FRECHET_PROJ_DIM columns: RandomState(seed).normal / sqrt(OUTPUT_DIM), drawn once per
        evaluator (as _probe_projection, from a seed of its own)"""
        if self._frechet_matrix is None:
            rng = np.random.RandomState(int(self.S.get('SEED', 0)) + EVAL_SEED + FRECHET_SEED)
            P = rng.normal(size=(self.cfg.output_dim, FRECHET_PROJ_DIM)) / np.sqrt(float(self.cfg.output_dim))
            self._frechet_matrix = torch.as_tensor(P.astype(np.float32)).to(self.device)
        return self._frechet_matrix

    def _frechet_sets(self, batches, rows):
        """z = q_z and pz = as many fresh prior draws, built exactly as _score_sets builds them; xr / gxr = real_x / Generator(pz), minibatch
        by minibatch, taken to the unit pixel range and through _frechet_projection -- over the full minibatches, at most `rows` rows per
        set.  The images themselves do not stay.  Called inside the pass's guard, under its own noise state."""
        c = self.cfg
        X, _ = self._stage(batches)
        B = c.B
        n = min(X.shape[0], max(1, int(rows) // B))
        new = lambda w: torch.empty((n * B, w), dtype=torch.float32, device=self.device)
        sets = dict(z=new(c.dim_latent), pz=new(c.dim_latent), xr=new(FRECHET_PROJ_DIM), gxr=new(FRECHET_PROJ_DIM))
        proj = self._frechet_projection()
        lo = 0.0 if c.out_act == 'sigmoid' else -1.0                      # (as _to_unit)

        def projected(x):
            x = x.float().reshape(B, -1).contiguous()
            if lo:
                x = F.Axpby.apply(x, None, 1.0 / (1.0 - lo), 0.0, -lo / (1.0 - lo))
            return F.Gemm.apply(x, proj, None, False, False, F.ACT_NONE, 0.0)
        self.kept = []
        for i in range(n):
            at = slice(i * B, (i + 1) * B)
            self._load(X[i])
            real_x = self.model.real_x(self.feed)
            q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if c.agg else self.model.Extractor(real_x)
            sets['z'][at].copy_(q[0] if isinstance(q, tuple) else q)
            sets['xr'][at].copy_(projected(real_x))
            p_z = self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']) if c.K else self.feed['p_z_noise']
            sets['pz'][at].copy_(p_z)
            sets['gxr'][at].copy_(projected(self.model.Generator(sets['pz'][at])))
        return sets

    def frechet_scores(self, batches, return_sets=False):
        """{'dev frechet z', 'dev frechet mean z', 'dev frechet xr', 'dev frechet mean xr'}: the Frechet distance between Gaussians fitted
        to two sets (functional.frechet_distance: |dmu|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), fp64 behind the moments, singular
        covariances allowed, not clipped at 0) -- z: q_z of the dev images against as many prior draws (through HyperGenerator with a mixture
        prior), the sets of `dev mmd z`; xr: the dev images against as many generated ones, pixels in [0, 1], both through one fixed random
        projection to FRECHET_PROJ_DIM = 128 columns whatever DIM_LATENT is.  The `mean` rows are the |dmu|^2 part of the row in front of
        them.  Over the full dev minibatches, at most FRECHET_MAX_ROWS rows per set and at least two.  The pass draws from a noise state of
        its own, swapped into the feed while it runs: every other pass logs the same values, and training reaches the same weights, whether
        it is on or not.  ONE host synchronisation; a raised status word (a non-finite moment: a diverged model; an eigenvalue iteration
        that did not converge) gives nan for that pair of rows and one printed message, no exception.  It fits GAUSSIANS, it is biased
        upward by about d^2 / n -- compare figures at equal row counts --, and xr is not comparable with any published FID.
        return_sets: (values, {z, pz, xr, gxr}: the device rows)."""
        S = self.S
        rows = int(S.get('FRECHET_MAX_ROWS', FRECHET_MAX_ROWS))
        if rows > F.FRECHET_MAX_ROWS:
            raise ValueError('FRECHET_MAX_ROWS = %d: at most %d rows per set' % (rows, F.FRECHET_MAX_ROWS))
        if self.cfg.dim_latent > F.FRECHET_MAX_DIM:
            raise ValueError('the Frechet pass takes at most %d columns, DIM_LATENT is %d' % (F.FRECHET_MAX_DIM, self.cfg.dim_latent))
        with self._guard():
            if self._frechet_rng is None:
                self._frechet_rng = F.noise_state(self.device, int(S.get('SEED', 0)) + EVAL_SEED + FRECHET_SEED)
            shared, self.feed['rng_state'] = self.feed['rng_state'], self._frechet_rng
            try:
                sets = self._frechet_sets(batches, rows)
            finally:
                self.feed['rng_state'] = shared
            if sets['z'].shape[0] < 2:
                raise ValueError('the Frechet pass needs at least 2 rows per set')
            (vz, sz), (vx, sx) = F.frechet_distance(sets['z'], sets['pz']), F.frechet_distance(sets['xr'], sets['gxr'])
            host = torch.cat([vz[:2], vx[:2], sz.double(), sx.double()]).cpu().numpy()
        status = (int(host[4]), int(host[5]))
        if any(status):
            print('[evaluate] frechet: status %d (z) / %d (xr) -- %d: a non-finite moment or entry, %d: the eigenvalue iteration did not converge '
                  '-- its values are nan' % (status[0], status[1], F.FRECHET_NONFINITE, F.FRECHET_NOT_CONVERGED))
        res = {k: (float('nan') if status[i // 2] else float(host[i])) for i, k in enumerate(FRECHET_KEYS)}
        return (res, sets) if return_sets else res

    _swd_rng = _swd_thetas = None             # the sliced-Wasserstein pass's own noise state and direction matrices, made by its first call

    def _swd_directions(self, L):
        """(theta_z [DIM_LATENT, L], theta_x [OUTPUT_DIM, L]): random unit directions, RandomState(seed).normal -- the latent matrix first,
        then the pixel matrix --, every column normalised in float64 and then cast to float32; drawn once per evaluator"""
        if self._swd_thetas is None or self._swd_thetas[0].shape[1] != L:
            rng = np.random.RandomState(int(self.S.get('SEED', 0)) + EVAL_SEED + SWD_SEED)
            made = []
            for d in (self.cfg.dim_latent, self.cfg.output_dim):
                t = rng.normal(size=(d, L))
                t /= np.sqrt(np.sum(t * t, axis=0, keepdims=True))
                made.append(torch.as_tensor(t.astype(np.float32)).to(self.device))
            self._swd_thetas = tuple(made)
        return self._swd_thetas

    def _swd_sets(self, batches, rows, L):
        """z = q_z, pz = as many fresh prior draws, real and generated images built exactly as _frechet_sets builds them, over the full
        minibatches, at most `rows` rows per set -- each minibatch projected at once onto its directions into its rows of a [rows, L]
        buffer: the pass holds four [rows, L] arrays whatever OUTPUT_DIM is, and the images do not stay.  Called inside the pass's guard,
        under its own noise state."""
        c = self.cfg
        X, _ = self._stage(batches)
        B = c.B
        n = min(X.shape[0], max(1, int(rows) // B))
        theta_z, theta_x = self._swd_directions(L)
        new = lambda: torch.empty((n * B, L), dtype=torch.float32, device=self.device)
        sets = dict(z_proj=new(), pz_proj=new(), x_proj=new(), gx_proj=new(), theta_z=theta_z, theta_x=theta_x)
        lo = 0.0 if c.out_act == 'sigmoid' else -1.0                      # (as _to_unit)

        def pixels(x):
            x = x.float().reshape(B, -1).contiguous()
            if lo:
                x = F.Axpby.apply(x, None, 1.0 / (1.0 - lo), 0.0, -lo / (1.0 - lo))
            return F.Gemm.apply(x, theta_x, None, False, False, F.ACT_NONE, 0.0)
        codes = lambda z: F.Gemm.apply(z.float().contiguous(), theta_z, None, False, False, F.ACT_NONE, 0.0)
        self.kept = []
        for i in range(n):
            at = slice(i * B, (i + 1) * B)
            self._load(X[i])
            real_x = self.model.real_x(self.feed)
            q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if c.agg else self.model.Extractor(real_x)
            sets['z_proj'][at].copy_(codes(q[0] if isinstance(q, tuple) else q))
            sets['x_proj'][at].copy_(pixels(real_x))
            p_z = self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']) if c.K else self.feed['p_z_noise']
            sets['pz_proj'][at].copy_(codes(p_z))
            sets['gx_proj'][at].copy_(pixels(self.model.Generator(p_z.contiguous())))
        return sets

    def swd_scores(self, batches, return_sets=False):
        """{'dev swd z', 'dev swd max z', 'dev swd x', 'dev swd max x'}: the sliced Wasserstein distance (functional.
        sliced_wasserstein_projected: per direction W_p^p between the two sorted columns, sorted on the device, fp64 behind the float32
        projections) over SWD_DIRS fixed random unit directions, p = SWD_P -- z: q_z of the dev images against as many prior draws (through
        HyperGenerator with a mixture prior), the sets of `dev mmd z`; x: the dev images against as many generated ones in the full pixel
        space, pixels in [0, 1].  The first row of a pair is (the mean over the directions)^(1/p), the `max` row (the largest)^(1/p), a lower
        bound of the max-sliced distance: it shows whether the discrepancy sits in a few directions.  Over the full dev minibatches, at
        most SWD_MAX_ROWS rows per set.  The pass draws from a noise state of its own, swapped into the feed while it runs: every other
        pass logs the same values, and training reaches the same weights, whether it is on or not.  ONE host synchronisation; a raised
        status word (a non-finite projection: a diverged model) gives nan for that pair of rows and one printed message, no exception.
        A Monte-Carlo estimate over directions fixed per seed -- compare figures at equal directions and row counts --, in pixel space,
        not comparable with any published SWD.
        return_sets: (values, {z_proj, pz_proj, x_proj, gx_proj: the projected device rows [rows, L]; theta_z, theta_x: the directions})."""
        S = self.S
        rows, L, p = int(S.get('SWD_MAX_ROWS', SWD_MAX_ROWS)), int(S.get('SWD_DIRS', SWD_DIRS)), int(S.get('SWD_P', SWD_P))
        if not 1 <= rows <= F.SWD_MAX_ROWS:
            raise ValueError('SWD_MAX_ROWS = %d: 1 to %d rows per set' % (rows, F.SWD_MAX_ROWS))
        if not 1 <= L <= F.SWD_MAX_DIRS:
            raise ValueError('SWD_DIRS = %d: 1 to %d directions' % (L, F.SWD_MAX_DIRS))
        if p not in (1, 2):
            raise ValueError('SWD_P = %d: 1 or 2' % p)
        with self._guard():
            if self._swd_rng is None:
                self._swd_rng = F.noise_state(self.device, int(S.get('SEED', 0)) + EVAL_SEED + SWD_SEED)
            shared, self.feed['rng_state'] = self.feed['rng_state'], self._swd_rng
            try:
                sets = self._swd_sets(batches, rows, L)
            finally:
                self.feed['rng_state'] = shared
            (vz, _, sz), (vx, _, sx) = (F.sliced_wasserstein_projected(sets['z_proj'], sets['pz_proj'], p),
                                        F.sliced_wasserstein_projected(sets['x_proj'], sets['gx_proj'], p))
            host = torch.cat([vz, vx, sz.double(), sx.double()]).cpu().numpy()
        status = (int(host[4]), int(host[5]))
        if any(status):
            print('[evaluate] swd: status %d (z) / %d (x) -- %d: a non-finite projected value -- its values are nan'
                  % (status[0], status[1], F.SWD_NONFINITE))
        res = {k: (float('nan') if status[i // 2] else float(host[i])) for i, k in enumerate(SWD_KEYS)}
        return (res, sets) if return_sets else res

    _cls_rng = _cls = None                    # the classifier pass's own noise state and its fitted classifier, made by its first call
    cls_fits = 0                              # how many times this evaluator fitted a classifier (a loaded file counts as none)

    def _cls_rows(self, batches, rows):
        """the leading full labelled minibatches, at most `rows` rows, as the classifier takes them: [(real_x float32 [B, OUTPUT_DIM], y int32
        [B])] on the device (copies: real_x may be the feed buffer itself)"""
        B = self.cfg.B
        full = [b for b in batches if _split(b)[0].shape[0] == B]
        if not full:
            raise ValueError('no full minibatch of %d rows to evaluate on' % B)
        n = min(len(full), max(1, int(rows) // B))
        out = []
        for s0 in range(0, n, max(1, PROBE_SLAB_ROWS // B)):
            X, Y = self._stage(full[s0:min(n, s0 + max(1, PROBE_SLAB_ROWS // B))], want_labels=True)
            for i in range(X.shape[0]):
                self.model.set_batch(self.feed, X[i])
                out.append((self.model.real_x(self.feed).float().reshape(B, -1).clone(), Y[i * B:(i + 1) * B]))
        return out

    def _classifier(self, fit_batches, classes):
        """the evaluator's classifier: the first call loads $GGAN_CLS_CKPT if that file exists, else fits one on the leading CLS_FIT_ROWS
        labelled training rows for CLS_EPOCHS epochs -> (classifier, fitted just now)"""
        if self._cls is not None:
            if self._cls.classes != classes:
                raise ValueError('the classifier was made for %d classes, these minibatches have %d' % (self._cls.classes, classes))
            return self._cls, False
        from .classifier import ImageClassifier
        S = self.S
        cls = ImageClassifier(self.cfg, classes, int(S.get('SEED', 0)) + EVAL_SEED + CLS_SEED, device=self.device)
        path = os.environ.get('GGAN_CLS_CKPT')
        fitted = not (path and os.path.exists(path))
        if fitted:
            cls.fit(self._cls_rows(fit_batches, S.get('CLS_FIT_ROWS', CLS_FIT_ROWS)), int(S.get('CLS_EPOCHS', CLS_EPOCHS)))
            self.cls_fits += 1
        else:
            cls.load(path)
        self._cls = cls
        return cls, fitted

    def classifier_scores(self, fit_batches, dev_batches, return_sets=False):
        """{'dev classifier score x', 'dev classifier score std x', 'dev classifier score data', 'dev classifier accuracy', 'dev classifier
        frechet x'}: the reference's one number about its samples (gan_inference_cifar10.py:381-391,483-487: 50000 images from fresh prior
        noise through a classifier, `inception score` and its std over ten splits, tflib/inception_score.py:47-53) under a classifier this
        run fits for itself (classifier.ImageClassifier: the Extractor's conv stack without BatchNorm, fitted on the leading CLS_FIT_ROWS
        labelled TRAINING rows for CLS_EPOCHS epochs) instead of the Inception graph the reference downloads.  score x / score std x:
        functional.class_score of the logits of floor(CLS_SAMPLES / B) generated minibatches (through HyperGenerator with a mixture prior)
        over CLS_SPLITS splits; score data: the same on at most CLS_MAX_ROWS labelled dev rows, the ceiling this classifier allows;
        accuracy: its accuracy on those rows, how far to trust the others; frechet x: functional.frechet_distance of its 128-wide
        features, the dev rows against as many generated rows.  Only logits and features stay on the device, never the images.
        The first call makes the classifier and keeps it (with $GGAN_CLS_CKPT = path: loads that file if it exists, else writes the fitted
        classifier there, so that two runs can be scored by ONE classifier -- figures under two classifiers do not compare); later calls,
        and the other set of weights under EMA_EVAL = both, reuse it.  The pass draws from a noise state of its own, swapped into the feed
        while it runs: every other pass logs the same values, and training reaches the same weights, whether it is on or not.  ONE host
        synchronisation per pass (the call that fits also copies the weights out when it writes the file); a raised status word (a label out
        of range, a non-finite logit or moment: a diverged model) gives nan and one printed message, no exception.  Not comparable with any
        published inception score or FID.
        return_sets: (values, {scores_x, scores_data: the per-split scores; entropies_x, entropies_data: (mean row entropy, entropy of the
        marginal); logits_x, features_x, logits_data, features_data, labels: the device rows; classifier})."""
        S, c = self.S, self.cfg
        B = c.B
        samples, rows, splits = int(S.get('CLS_SAMPLES', CLS_SAMPLES)), int(S.get('CLS_MAX_ROWS', CLS_MAX_ROWS)), int(S.get('CLS_SPLITS', CLS_SPLITS))
        if not B <= samples <= F.CLS_SCORE_MAX_ROWS:
            raise ValueError('CLS_SAMPLES = %d: one minibatch (%d) to %d rows' % (samples, B, F.CLS_SCORE_MAX_ROWS))
        if not 2 <= rows <= min(F.CLS_MAX_BATCH, F.FRECHET_MAX_ROWS):
            raise ValueError('CLS_MAX_ROWS = %d: 2 to %d rows' % (rows, min(F.CLS_MAX_BATCH, F.FRECHET_MAX_ROWS)))
        if not 1 <= splits <= F.CLS_MAX_SPLITS:
            raise ValueError('CLS_SPLITS = %d: 1 to %d splits' % (splits, F.CLS_MAX_SPLITS))
        labels = [_split(b)[1] for b in list(fit_batches) + list(dev_batches)]
        if not fit_batches or not dev_batches or any(y is None for y in labels):
            raise ValueError('the classifier pass needs labelled minibatches on both sides')
        classes = max(2, 1 + max(int(y.max()) for y in labels))      # (host labels: no device is asked)
        if classes > F.CLS_MAX_CLASSES:
            raise ValueError('the classifier takes at most %d classes, got %d' % (F.CLS_MAX_CLASSES, classes))
        with self._guard():
            if self._cls_rng is None:
                self._cls_rng = F.noise_state(self.device, int(S.get('SEED', 0)) + EVAL_SEED + CLS_SEED)
            shared, self.feed['rng_state'] = self.feed['rng_state'], self._cls_rng
            try:
                cls, fitted = self._classifier(fit_batches, classes)
                n = samples // B
                new = lambda r, w: torch.empty((r, w), dtype=torch.float32, device=self.device)
                gl, gf = new(n * B, classes), new(n * B, cls.params['Feature.W'].shape[1])
                for i in range(n):
                    self.model.sample_noise(self.feed)
                    p_z = self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']) if c.K else self.feed['p_z_noise']
                    lg, ft = cls.logits(self.model.Generator(p_z), features=True)
                    gl[i * B:(i + 1) * B].copy_(lg)
                    gf[i * B:(i + 1) * B].copy_(ft)
                dev = self._cls_rows(dev_batches, rows)
                m = len(dev) * B
                dl, df, dy = new(m, classes), new(m, gf.shape[1]), torch.cat([y for _, y in dev])
                for i, (x, _) in enumerate(dev):
                    lg, ft = cls.logits(x, features=True)
                    dl[i * B:(i + 1) * B].copy_(lg)
                    df[i * B:(i + 1) * B].copy_(ft)
                del dev
            finally:
                self.feed['rng_state'] = shared
            if m < 2 or n * B < 2:
                raise ValueError('the classifier pass needs at least 2 rows per set')
            sx, sd = F.class_score(gl, min(splits, n * B)), F.class_score(dl, min(splits, m))
            _, hits, st_y = F.softmax_xent(dl, dy)
            both = min(m, n * B)                                     # as many rows on either side
            fd, st_f = F.frechet_distance(df[:both], gf[:both])
            host = torch.cat([sx.mean.reshape(1).double(), sx.std.reshape(1).double(), sd.mean.reshape(1).double(), hits.double(), fd[:1],
                              sx.status.double(), sd.status.double(), st_y.double(), st_f.double()]).cpu().numpy()
        status = (int(host[5]), int(host[5]), int(host[6]), int(host[7]), int(host[8]) | int(host[5]) | int(host[6]))
        if any(status):
            print('[evaluate] classifier: status %d (x) / %d (data) / %d (accuracy) / %d (frechet) -- scores and accuracy: %d a label out of '
                  'range, %d a non-finite logit; frechet: %d a non-finite moment, %d the eigenvalue iteration did not converge -- its values '
                  'are nan' % (status[0], status[2], status[3], int(host[8]), F.CLS_BAD_LABEL, F.CLS_NONFINITE, F.FRECHET_NONFINITE,
                               F.FRECHET_NOT_CONVERGED))
        vals = (float(host[0]), float(host[1]), float(host[2]), float(host[3]) / m, float(host[4]))
        res = {k: (float('nan') if st else v) for k, v, st in zip(CLS_KEYS, vals, status)}
        if fitted:
            cls.held_out = res['dev classifier accuracy']
            path = os.environ.get('GGAN_CLS_CKPT')
            if path:
                cls.save(path)
        if return_sets:
            return res, dict(scores_x=sx.scores, scores_data=sd.scores, entropies_x=(sx.row_entropy, sx.marginal_entropy),
                             entropies_data=(sd.row_entropy, sd.marginal_entropy), logits_x=gl, features_x=gf, logits_data=dl, features_data=df,
                             labels=dy, classifier=cls)
        return res

    _km_rng = _km_bins = None                 # the k-means pass's own noise state and its fitted bins, made by its first call
    _km_said = False                          # the one message about unlabelled dev data was printed
    km_fits = 0                               # how many times this evaluator fitted the bins ...
    km_z_fits = 0                             # ... and the clusters of the codes

    def _km_unit(self, x):
        """[B, OUTPUT_DIM] in the Generator's range -> float32 pixels in [0, 1] (as _to_unit), on the device"""
        lo = 0.0 if self.cfg.out_act == 'sigmoid' else -1.0
        x = x.float().reshape(self.cfg.B, -1).contiguous()
        return F.Axpby.apply(x, None, 1.0 / (1.0 - lo), 0.0, -lo / (1.0 - lo)) if lo else x

    def _km_rows(self, batches, rows, codes=False):
        """the leading full minibatches, at most `rows` rows -> (pixels float32 [n B, OUTPUT_DIM] in [0, 1], q_z float32 [n B, DIM_LATENT] or
        None, int32 labels [n B] or None where a minibatch has none), on the device"""
        c, B = self.cfg, self.cfg.B
        full = [b for b in batches if _split(b)[0].shape[0] == B]
        if not full:
            raise ValueError('no full minibatch of %d rows to evaluate on' % B)
        n = min(len(full), max(1, int(rows) // B))
        labels = all(_split(b)[1] is not None for b in full[:n])
        X = torch.empty((n * B, c.output_dim), dtype=torch.float32, device=self.device)
        Z = torch.empty((n * B, c.dim_latent), dtype=torch.float32, device=self.device) if codes else None
        Y = []
        slab = max(1, PROBE_SLAB_ROWS // B)
        for s0 in range(0, n, slab):
            Xs, Ys = self._stage(full[s0:min(n, s0 + slab)], want_labels=labels)
            Y.append(Ys)
            for i in range(Xs.shape[0]):
                at = slice((s0 + i) * B, (s0 + i + 1) * B)
                if codes:
                    self._load(Xs[i])
                else:
                    self.model.set_batch(self.feed, Xs[i])
                real_x = self.model.real_x(self.feed)
                X[at].copy_(self._km_unit(real_x))
                if codes:
                    q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if c.agg else self.model.Extractor(real_x)
                    Z[at].copy_((q[0] if isinstance(q, tuple) else q).float().reshape(B, -1))
        return X, Z, (torch.cat(Y) if labels else None)

    def _km_uniforms(self, k, which):
        """the k uniforms of a seeding, drawn on the host from a RandomState of the pass's own: 0 the bins, 1 the clusters of the codes"""
        return np.random.RandomState(int(self.S.get('SEED', 0)) + EVAL_SEED + KM_SEED + which).rand(k)

    def kmeans_scores(self, fit_batches, dev_batches, return_sets=False):
        """{'dev ndb x', 'dev ndb js x', 'dev ndb data', 'dev kmeans accuracy z', 'dev kmeans nmi z'}: which regions of the data the Generator
        over- or under-populates, and whether the classes form clusters in the code space; nothing of it exists in the reference.
        ndb x / ndb js x: NDB/K of Richardson & Weiss 2018 -- functional.kmeans_fit cuts the pixel space ([0, 1] pixels, Euclidean cells) into
        KM_BINS Voronoi cells on the leading KM_FIT_ROWS training rows, floor(KM_SAMPLES / B) generated minibatches (through HyperGenerator
        with a mixture prior) are assigned to the cells a slab at a time, only the counts stay, and functional.bin_test gives the share of
        cells whose two-proportion z statistic exceeds KM_Z_THRESHOLD and the Jensen-Shannon divergence of the two histograms; ndb data: the
        same share for at most KM_MAX_ROWS dev images, the floor the statistic has on real data.  kmeans accuracy z / kmeans nmi z: a second
        k-means on q_z of the labelled dev rows, KM_Z_CLUSTERS clusters (N_COMS under a mixture prior, else the classes seen), then
        functional.cluster_scores: purity (every cluster takes its majority label) and NMI; unlabelled dev data: the two rows are left
        out with one message.  The bins are fitted ONCE per evaluator, at the first call (they depend on the data and the seed, not on the
        model); the clusters of the codes at every call.  The pass draws from a noise state of its own, swapped into the feed while it runs:
        every other pass logs the same values, and training reaches the same weights, whether it is on or not.  ONE host synchronisation; a
        raised status word (a non-finite pixel or code: a diverged model) gives nan for the rows it touches and one printed message.
        return_sets: (values, {centres, counts_fit, counts_x, counts_data, moved, inertia: the bins' fit; and with labels centres_z, assign_z,
        moved_z, inertia_z, labels, table})."""
        S, c = self.S, self.cfg
        B = c.B
        bins, fit_rows, samples = int(S.get('KM_BINS', KM_BINS)), int(S.get('KM_FIT_ROWS', KM_FIT_ROWS)), int(S.get('KM_SAMPLES', KM_SAMPLES))
        rows, iters, zthr = int(S.get('KM_MAX_ROWS', KM_MAX_ROWS)), int(S.get('KM_ITERS', KM_ITERS)), float(S.get('KM_Z_THRESHOLD', KM_Z_THRESHOLD))
        if not 1 <= bins <= F.KMEANS_MAX_K:
            raise ValueError('KM_BINS = %d: 1 to %d bins' % (bins, F.KMEANS_MAX_K))
        if not B <= fit_rows <= F.KMEANS_MAX_ROWS:
            raise ValueError('KM_FIT_ROWS = %d: one minibatch (%d) to %d rows' % (fit_rows, B, F.KMEANS_MAX_ROWS))
        if samples < B:
            raise ValueError('KM_SAMPLES = %d: at least one minibatch (%d)' % (samples, B))
        if not B <= rows <= F.KMEANS_MAX_ROWS:
            raise ValueError('KM_MAX_ROWS = %d: one minibatch (%d) to %d rows' % (rows, B, F.KMEANS_MAX_ROWS))
        if not 0 <= iters <= F.KMEANS_MAX_ITERS:
            raise ValueError('KM_ITERS = %d: 0 to %d iterations' % (iters, F.KMEANS_MAX_ITERS))
        if not fit_batches or not dev_batches:
            raise ValueError('the k-means pass needs training minibatches for its bins and dev minibatches')
        labels = [_split(b)[1] for b in dev_batches]
        labelled = all(y is not None for y in labels)
        classes = kz = 0
        if labelled:
            classes = max(2, 1 + max(int(np.asarray(y.cpu() if torch.is_tensor(y) else y).max()) for y in labels))      # (host labels: no device is asked)
            if classes > F.KMEANS_MAX_CLASSES:
                raise ValueError('the clustering scores take at most %d classes, got %d' % (F.KMEANS_MAX_CLASSES, classes))
            kz = int(S.get('KM_Z_CLUSTERS') or (c.K if c.K else classes))
            if not 1 <= kz <= F.KMEANS_MAX_K:
                raise ValueError('KM_Z_CLUSTERS = %d: 1 to %d clusters' % (kz, F.KMEANS_MAX_K))
        elif not self._km_said:
            print('[evaluate] dev kmeans accuracy z / nmi z skipped: no labelled dev set')
            self._km_said = True
        zero = lambda k: torch.zeros((k,), dtype=torch.int32, device=self.device)
        with self._guard():
            if self._km_rng is None:
                self._km_rng = F.noise_state(self.device, int(S.get('SEED', 0)) + EVAL_SEED + KM_SEED)
            shared, self.feed['rng_state'] = self.feed['rng_state'], self._km_rng
            try:
                if self._km_bins is None:
                    X, _, _ = self._km_rows(fit_batches, fit_rows)
                    self._km_bins = F.kmeans_fit(X, bins, iters, self._km_uniforms(bins, 0))
                    self.km_fits += 1
                    del X                                            # (the training images leave the device; stream-ordered)
                fit = self._km_bins
                n = samples // B
                slab = max(1, PROBE_SLAB_ROWS // B)
                counts_x, st_x = zero(bins), zero(1)
                buf = torch.empty((min(n, slab) * B, c.output_dim), dtype=torch.float32, device=self.device)
                for s0 in range(0, n, slab):
                    m = min(slab, n - s0)
                    for i in range(m):
                        self.model.sample_noise(self.feed)
                        p_z = self.model.HyperGenerator(self.feed['k_onehot'], self.feed['p_z_noise']) if c.K else self.feed['p_z_noise']
                        buf[i * B:(i + 1) * B].copy_(self._km_unit(self.model.Generator(p_z.contiguous())))
                    st_x |= F.kmeans_assign(buf[:m * B], fit.centres, counts=counts_x)[4]
                del buf
                X, Z, Y = self._km_rows(dev_batches, rows, codes=labelled)
                counts_d = zero(bins)
                st_d = F.kmeans_assign(X, fit.centres, counts=counts_d)[4]
                del X
                zfit = None
                if labelled:
                    zfit = F.kmeans_fit(Z, kz, iters, self._km_uniforms(kz, 1))
                    self.km_z_fits += 1
                    zs, table, st_c = F.cluster_scores(zfit.assign, Y, kz, classes)
            finally:
                self.feed['rng_state'] = shared
            ndb_x, ndb_d = F.bin_test(fit.counts, counts_x, zthr), F.bin_test(fit.counts, counts_d, zthr)
            parts = [ndb_x[1:], ndb_d[1:2], (fit.status | st_x).double(), (fit.status | st_d).double()]
            if labelled:
                parts += [zs, (zfit.status | st_c).double()]
            host = torch.cat(parts).cpu().numpy()
        status = (int(host[3]), int(host[3]), int(host[4])) + ((int(host[7]), int(host[7])) if labelled else ())
        if any(status):
            print('[evaluate] kmeans: status %d (x) / %d (data)%s -- %d: a non-finite pixel, code or distance, %d: a label or an assignment '
                  'out of range -- its values are nan' % (status[0], status[2], ' / %d (z)' % status[3] if labelled else '', F.KMEANS_NONFINITE,
                                                          F.KMEANS_BAD_INDEX))
        vals = (float(host[0]), float(host[1]), float(host[2])) + ((float(host[5]), float(host[6])) if labelled else ())
        res = {k: (float('nan') if st else v) for k, v, st in zip(KM_KEYS, vals, status)}
        if return_sets:
            sets = dict(centres=fit.centres, counts_fit=fit.counts, counts_x=counts_x, counts_data=counts_d, moved=fit.moved, inertia=fit.inertia)
            if labelled:
                sets.update(centres_z=zfit.centres, assign_z=zfit.assign, moved_z=zfit.moved, inertia_z=zfit.inertia, labels=Y, table=table,
                            codes=Z)
            return res, sets
        return res

    def manifold(self, batches, out_dir, frame):
        """embeds the point sets of latent_sets with functional.tsne and writes the scatters under the reference's file names; returns
        the paths: the four pictures of gmgan_inference_mnist with a mixture prior, the one of gan_inference_mnist without.  MNIST models
        only (the reference draws them in no other script).  self.manifold_log: (point set, KL, seconds) of each embedding, also printed.  MANIFOLD_PERPLEXITY (30) and
        MANIFOLD_ITERS (1000) of the settings reach the embedder; its initial positions are seeded from the settings seed."""
        c = self.cfg
        if c.dataset != 'mnist':
            raise ValueError('the latent-space pictures are a pass of the MNIST scripts (%s); dataset %r has none' % (', '.join(MANIFOLD_SCRIPTS), c.dataset))
        sets = self.latent_sets(batches)
        t_sets = self.last_seconds
        mode = self.S.get('MODE', c.mode)
        perplexity, n_iter = float(self.S.get('MANIFOLD_PERPLEXITY', 30.)), int(self.S.get('MANIFOLD_ITERS', 1000))
        seed = int(self.S.get('SEED', 0)) + EVAL_SEED
        paths, embedded, self.manifold_log = [], {}, []
        with self._guard():
            for fname, points, labels in (_MANIFOLD_K if c.K else _MANIFOLD):
                if points not in embedded:
                    t0 = time.time()
                    Y, kl = F.tsne(sets[points], perplexity=perplexity, n_iter=n_iter, seed=seed, return_kl=True)
                    embedded[points] = Y.cpu().numpy()
                    self.manifold_log.append((points, kl, time.time() - t0))
                    print('[eval] t-SNE of %s %s: KL %.4f, %.2f s' % (points, tuple(sets[points].shape), kl, time.time() - t0))
                out_name = self._fname(fname.format(frame=frame, mode=mode))
                lib.visualization.scatter(embedded[points], sets[labels].cpu().numpy(), out_dir, out_name)
                paths.append(os.path.join(out_dir, out_name))
        self.last_seconds += t_sets
        return paths

    def _to_unit(self, x):
        """generator output -> [0, 1] images for save_images"""
        lo = 0.0 if self.cfg.out_act == 'sigmoid' else -1.0
        return np.clip((x - lo) / (1.0 - lo), 0, 1)

    def sample_grid(self):
        """the fixed-noise samples of generate_image -> numpy [N_VIS, OUTPUT_DIM] (generator output range).  gmgan: row r is component
        r % N_COMS, so that a grid of N_VIS / N_COMS rows and N_COMS columns has one component per column."""
        with self._guard():
            p_z = self.model.HyperGenerator(self.fixed_k, self.fixed_noise) if self.cfg.K else self.fixed_noise
            return self.model.Generator(p_z).float().cpu().numpy()

    def set_fixed_data(self, batch):
        images, _ = _split(batch)
        self.fixed_data = np.asarray(images.cpu() if torch.is_tensor(images) else images).reshape(self.cfg.B, -1)

    def reconstructions(self, batch=None):
        """reconstruct_image: (real [B, D], Generator(Extractor(real)) [B, D]) on the fixed dev minibatch, as numpy"""
        if batch is not None:
            self.set_fixed_data(batch)
        assert self.fixed_data is not None, 'no reconstruction minibatch: pass one or call set_fixed_data'
        with self._guard():
            X, _ = self._stage([self.fixed_data])
            self.model.set_batch(self.feed, X[0])
            self.model.sample_noise(self.feed)
            real_x = self.model.real_x(self.feed)
            q = self.model.Extractor(real_x, eps=self.feed['q_eps']) if self.cfg.agg else self.model.Extractor(real_x)
            q_z = q[0] if isinstance(q, tuple) else q
            rec = self.model.Generator(q_z)
            return real_x.float().cpu().numpy(), rec.float().cpu().numpy()

    def save_images(self, out_dir, frame, script=None):
        """writes the sample grid and the reconstruction pairs under the reference's file names; returns the paths"""
        c = self.cfg
        name = os.path.splitext(os.path.basename(script or self.S.get('SCRIPT', '')))[0]
        fs, fr = _NAMES.get(name, _DEFAULT_NAMES_K if c.K else _DEFAULT_NAMES)
        mode = self.S.get('MODE', c.mode)
        shape = (-1, c.C, c.S, c.S)
        paths = []
        grid = self._to_unit(self.sample_grid()).reshape(shape)
        p = self._fname(os.path.join(out_dir, fs.format(frame=frame, mode=mode)))
        lib.save_images.save_images(grid, p, size=[grid.shape[0] // c.K, c.K] if c.K else None)
        paths.append(p)
        if self.fixed_data is not None:
            real, rec = self.reconstructions()
            pairs = np.empty((2 * c.B, c.output_dim), dtype=np.float32)
            pairs[0::2], pairs[1::2] = self._to_unit(real), self._to_unit(rec)
            p = self._fname(os.path.join(out_dir, fr.format(frame=frame, mode=mode)))
            lib.save_images.save_images(pairs.reshape(shape), p)
            paths.append(p)
        return paths


# ---- the state-space scripts' video passes ---------------------------------------------------------------------------------------------
VIDEO_NAMES = ('samples', 'train_data', 'reconstruction', 'disentangle')


def pixel_maps(dataset):
    """(a, b, d) of ggan_video_sheet_u8: generated frames q = trunc(((x + 1) * a) * b), data q = trunc(x * d).
    chairs: int((x + 1) * (255.99 / 2)) (ssgan_inference_chairs.py:577), data the loader's 0..255 values.
    moving-MNIST: u = (x + 1) / 2 then save_images' uint8(255.99 * u) (:595), data in [0, 1] through the same uint8(255.99 * u); the
    script's (x + 1) * 2. of generate_video / disentangle (:586,:612) is NOT reproduced."""
    if dataset == 'chairs':
        return 255.99 / 2, 1.0, 1.0
    return 0.5, 255.99, 255.99


def host_sheet(gen, data, shape, maps, interleave=False):
    """the bytes ggan_video_sheet_u8 produces, on the host in numpy float32 in the written order (the old way: floats downloaded,
    large_image's tiling loop) -> (sheet [rows*H, LEN*W, C], index planes [LEN, nh*H, nw*W])"""
    a, b, d = (np.float32(v) for v in maps)
    q = lambda v: np.clip(np.trunc(v), 0, 255).astype(np.uint8)
    parts = []
    if data is not None:
        parts.append(q(np.asarray(data, np.float32) * d))
    if gen is not None:
        parts.append(q(((np.asarray(gen, np.float32) + np.float32(1)) * a) * b))
    n, LEN = parts[0].shape[:2]
    if interleave:
        x = np.empty((2 * n, LEN) + tuple(shape), np.uint8)
        x[0::2], x[1::2] = parts[0].reshape((n, LEN) + tuple(shape)), parts[1].reshape((n, LEN) + tuple(shape))
    else:
        assert len(parts) == 1
        x = parts[0].reshape((n, LEN) + tuple(shape))
    rows = x.shape[0]
    sheet = lib.save_images.large_image(x.reshape((-1,) + tuple(shape)), size=(rows, LEN))
    planes, _ = lib.save_images.gif_planes(x)
    return sheet, planes


class SequenceEvaluator(_Passes):
    def __init__(self, trainer, settings):
        """trainer: an engine.Trainer of a state-space script (models_ssgan.StateSpaceGAN); settings: the script's UPPERCASE block
        (BATCH_SIZE, N_VIS, SEED).  The fixed inputs are drawn once, in the reference's order, from a generator of the evaluator's own."""
        self.tr, self.S = trainer, settings
        self.model, self.cfg, self.device = trainer.model, trainer.cfg, trainer.device
        c = self.cfg
        seed = int(settings.get('SEED', 0)) + EVAL_SEED
        n_vis = int(settings.get('N_VIS', c.B))
        # (the nets are built for BATCH_SIZE sequences: N_VIS = BATCH_SIZE, ssgan_inference_moving_mnist.py:55)
        assert n_vis == c.B, 'N_VIS must be BATCH_SIZE'
        assert not c.n_c or n_vis % c.n_c == 0, 'N_VIS must be a multiple of N_C (ssgan_inference_moving_mnist.py:56)'
        self.feed = self.model.feed_buffers(self.device)
        self.feed['rng_state'] = F.noise_state(self.device, seed)
        rng = np.random.RandomState(seed)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.pre_fixed_noise = up(rng.normal(size=(n_vis, c.dim_l)))                                    # :579
        self.fixed_y = up(np.tile(np.eye(c.n_c), (n_vis // c.n_c, 1)) if c.n_c else np.zeros((n_vis, 0)))        # :580
        self.fixed_noise_g = up(rng.normal(size=(n_vis, c.dim_g)))                                      # :581
        dis_y = np.zeros((c.B, c.n_c))
        if c.n_c:
            dis_y[:, 1] = 1                                                                               # :607 class 1 for every row
        self.dis_y = up(dis_y)
        self.dis_g = up(np.tile(rng.normal(size=(1, c.dim_g)), (c.B, 1)))                               # :608
        self.rec_data = self.dis_data = None          # the fixed dev minibatches (device: (x [B, LEN, D], one-hot y [B, N_C]))
        self.timing = {}                              # seconds of the last save_videos: device / download / encode

    # ---- plumbing ------------------------------------------------------------------------------------------------------------------
    def _batch(self, batch):
        """a loader minibatch (x, or (x, labels), labels as class numbers or one-hot rows; host or device) -> device (x, one-hot y)"""
        c = self.cfg
        x, y = _split(batch)
        x = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))).to(self.device, torch.float32)
        x = x.reshape(c.B, c.LEN, c.output_dim).clone()
        oh = torch.zeros((c.B, c.n_c), dtype=torch.float32, device=self.device)
        if c.n_c:
            if y is None:
                raise ValueError('the moving-MNIST passes need labelled minibatches')
            y = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))
            if y.dim() == 2:
                oh.copy_(y.to(self.device, torch.float32))
            else:
                oh[torch.arange(c.B, device=self.device), y.to(self.device, torch.int64)] = 1
        return x, oh

    def set_fixed_data(self, rec_batch, dis_batch=None):
        """the reconstruction minibatch and the disentangling one (each the first minibatch of a fresh dev generator, :591,:605)"""
        self.rec_data = self._batch(rec_batch)
        self.dis_data = self._batch(dis_batch) if dis_batch is not None else self.rec_data

    def _extract(self, data):
        """(real_y, q_z_g, q_z_l) of a fixed minibatch (:514-518), through the evaluator's own feed"""
        m = self.model
        m.set_batch(self.feed, data)
        u = self.feed['real_x_unit']
        real_x = F.Axpby.apply(u, u, 2.0 / self.cfg.x_div, 0.0, -1.0)                                  # 2*(x/div-.5)
        real_y = self.feed['real_y']
        return real_y, m.G_Extractor(real_x, real_y), m.DynamicExtractor(m.Extractor(real_x, real_y))

    # ---- the passes: device tensors [B, LEN, OUTPUT_DIM] in the generator's range -----------------------------------------------------
    def samples(self):
        """fixed_noise_samples (:582-583); epsilon is drawn anew on every call (:137) and stays in self.feed['epsilon']"""
        with self._guard():
            F.noise_fill_(self.feed['rng_state'], [(self.feed['epsilon'], F.NOISE_NORMAL, 0., 1.)])
            z_l = self.model.DynamicGenerator(self.pre_fixed_noise, self.feed['epsilon'])
            return self.model.Generator(self.fixed_noise_g, z_l, self.fixed_y)

    def reconstructions(self, batch=None):
        """rec_x = Generator(q_z_g, q_z_l, real_y) on the fixed minibatch (:519,:594)"""
        data = self._batch(batch) if batch is not None else self.rec_data
        assert data is not None, 'no reconstruction minibatch: pass one or call set_fixed_data'
        with self._guard():
            real_y, q_z_g, q_z_l = self._extract(data)
            return self.model.Generator(q_z_g, q_z_l, real_y)

    def disentangle(self, batch=None):
        """dis_x = Generator(dis_g, q_z_l, dis_y) (:609): one global code, the fixed minibatch's per-frame codes"""
        data = self._batch(batch) if batch is not None else self.dis_data
        assert data is not None, 'no disentangling minibatch: pass one or call set_fixed_data'
        with self._guard():
            _, _, q_z_l = self._extract(data)
            return self.model.Generator(self.dis_g, q_z_l, self.dis_y)

    def rec_scores(self, batches, return_rows=False, per_frame=False):
        """{'dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x'} of reconstructions(batch) against the data over the full
        dev minibatches, FRAME by frame (n = B * LEN rows per minibatch; at most REC_MAX_ROWS frames and at least one minibatch): the
        generated frames in the tanh range, the data in the loader's units, both mapped to [0, 1] inside the kernel's formula -- the
        per-frame figures the video-prediction literature reports.  functional.ssim_pairs per minibatch, the statistics in float64 on
        the device, ONE host synchronisation.  per_frame: the values also hold mse_t, psnr_t, ssim_t, the [LEN] means by frame index
        (numpy).  return_rows: (values, {mse, psnr, ssim}: the per-frame device rows, sequence-major).  The evaluator's own feed and
        noise state; the Trainer is left untouched."""
        c = self.cfg
        full = [b for b in batches if _split(b)[0].shape[0] == c.B]
        if not full:
            raise ValueError('no full minibatch of %d sequences to evaluate on' % c.B)
        full = full[:max(1, int(self.S.get('REC_MAX_ROWS', REC_MAX_ROWS)) // (c.B * c.LEN))]
        t0 = time.time()
        mse, ssim = [], []
        for b in full:
            data = self._batch(b)
            rec = self.reconstructions(data)
            with self._guard():
                m, s = F.ssim_pairs(rec.float(), data[0], (c.C, c.S, c.S), (0.5, 0.5), (1.0 / c.x_div, 0.0))
            mse.append(m)
            ssim.append(s)
        with self._guard():
            mse, ssim = torch.cat(mse), torch.cat(ssim)
            vals, psnr = _rec_stats(mse, ssim)
            if per_frame:
                vals = torch.cat([vals] + [v.double().view(-1, c.LEN).mean(dim=0) for v in (mse, psnr, ssim)])
            vals = vals.cpu().numpy()
        self.last_seconds = time.time() - t0
        res = {name: float(v) for name, v in zip(REC_KEYS, vals[:4])}
        if per_frame:
            for i, name in enumerate(('mse_t', 'psnr_t', 'ssim_t')):
                res[name] = vals[4 + i * c.LEN:4 + (i + 1) * c.LEN].copy()
        return (res, dict(mse=mse, psnr=psnr, ssim=ssim)) if return_rows else res

    # ---- files ---------------------------------------------------------------------------------------------------------------------
    def sheets(self, train_data=None):
        """{name: (sheet bytes, index planes)} on the device for the passes' files: one ggan_video_sheet_u8 launch each"""
        c = self.cfg
        shape, (a, b, d) = (c.C, c.S, c.S), pixel_maps(c.dataset)
        out = {}
        out['samples'] = F.video_sheet_u8(self.samples(), None, shape, a, b, d)
        if train_data is not None:
            x = _split(train_data)[0]
            out['train_data'] = F.video_sheet_u8(None, x.to(self.device, torch.float32).reshape(c.B, c.LEN, c.output_dim), shape, a, b, d)
        if self.rec_data is not None:
            out['reconstruction'] = F.video_sheet_u8(self.reconstructions(), self.rec_data[0], shape, a, b, d, interleave=True)
            out['disentangle'] = F.video_sheet_u8(self.disentangle(), self.dis_data[0], shape, a, b, d, interleave=True)
        return out

    def save_videos(self, out_dir, frame, train_data=None):
        """writes <name>_<frame>.png / .gif for samples, train_data (the minibatch handed in), reconstruction and disentangle; returns
        the paths.  Only the byte tensors are downloaded; self.timing splits the wall time into device / download / encode seconds."""
        S = lib.save_images
        t0 = time.time()
        dev = self.sheets(train_data)
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        t1 = time.time()
        host = {k: (s.cpu().numpy(), g.cpu().numpy()) for k, (s, g) in dev.items()}
        t2 = time.time()
        palette = S.grey_palette() if self.cfg.C == 1 else S.cube_palette()
        paths = []
        for name in VIDEO_NAMES:
            if name not in host:
                continue
            sheet, planes = host[name]
            # (train_data holds data only: one file whatever weights the other three were drawn from)
            stem = os.path.join(out_dir, '%s_%s' % (name, frame)) + ('_ema' if self.weights == 'ema' and name != 'train_data' else '')
            S.write_png(stem + '.png', sheet)
            S.write_gif(stem + '.gif', planes, palette)
            paths += [stem + '.png', stem + '.gif']
        self.timing = dict(device=t1 - t0, download=t2 - t1, encode=time.time() - t2)
        return paths


# ---- command line: score a saved checkpoint ----------------------------------------------------------------------------------------
def main(argv=None):
    """builds the script's model, restores the checkpoint's weights, runs the evaluation passes once and prints them"""
    from . import checkpoint, run
    from .engine import Trainer
    ap = argparse.ArgumentParser(prog='python -m graphical_gan_amd.evaluate', description=main.__doc__)
    ap.add_argument('ckpt', help='a params_<it>.npz written by run.train / checkpoint.save')
    ap.add_argument('--script', required=True, help='the script the checkpoint was trained with, e.g. gmgan_inference_mnist or ssgan_inference_chairs')
    ap.add_argument('--data-dir', default=os.environ.get('GGAN_DATA_DIR', ''))
    ap.add_argument('--mode', default=None, help="the script's MODE (default: the script's own)")
    ap.add_argument('--out-dir', default=None, help='also write the sample grid and the reconstructions here (the state-space scripts: the video files, required)')
    ap.add_argument('--manifold', action='store_true', help='also write the latent-space t-SNE pictures of the MNIST scripts to --out-dir')
    for row in SET_SCORES:
        ap.add_argument('--' + row.name, action='store_true', help=row.help)
    ap.add_argument('--probe', action='store_true', help='also fit a least-squares linear probe on the codes of labelled training rows and score it on the labelled dev set (dev probe accuracy z / fit probe accuracy z / dev probe accuracy xr; image scripts with labelled data)')
    ap.add_argument('--probe-wide', action='store_true', help='implies --probe; also fit the same probe on the pixels themselves and on the top activations of the Extractor (dev / fit probe accuracy x and h; up to 4096 columns)')
    ap.add_argument('--frechet', action='store_true', help='also score the dev set by the Frechet distance between Gaussians fitted to q_z and prior draws, and to randomly projected dev and generated images (dev frechet z / xr and their mean parts; image scripts; not comparable with a published FID)')
    ap.add_argument('--swd', action='store_true', help='also score the dev set by the sliced Wasserstein distance of q_z against prior draws and of the dev images against generated ones in the full pixel space, over fixed random unit directions (dev swd z / x and their max rows; image scripts; not comparable with a published SWD)')
    ap.add_argument('--cls', action='store_true', help='also score 50000 generated images by the inception-score formula under a small classifier fitted on the labelled training rows (or loaded from $GGAN_CLS_CKPT), with the same score of the dev images, its accuracy and the Frechet distance of its features (dev classifier score x / score std x / score data / accuracy / frechet x; image scripts with labelled data; not comparable with a published inception score or FID)')
    ap.add_argument('--kmeans', action='store_true', help='also bin 20000 generated images into k-means cells fitted on the device on the leading training rows and report NDB/K, the Jensen-Shannon divergence of the two histograms and the NDB/K of the dev images, and score a k-means of q_z of the labelled dev set by purity and NMI (dev ndb x / ndb js x / ndb data / kmeans accuracy z / kmeans nmi z; image scripts; the z rows need labels; comparable with published NDB figures only at equal K, row counts and space)')
    ap.add_argument('--ema', action='store_true', help="score the averaged generator-side weights the checkpoint holds (its ema/gen/ keys, written by a run with $GGAN_EMA_DECAY) instead of the last iterate: every name gets the suffix ' ema', every file '_ema'; the critic of 'dev gen cost ema' is the live one")
    ap.add_argument('--set', action='append', default=[], metavar='KEY=VALUE', help='override an UPPERCASE setting (int / float / str)')
    a = ap.parse_args(argv)
    over = {}
    for kv in a.set:
        k, v = kv.split('=', 1)
        for conv in (int, float):
            try:
                v = conv(v)
                break
            except ValueError:
                pass
        over[k] = v
    if a.mode:
        over['MODE'] = a.mode
    if os.path.splitext(os.path.basename(a.script))[0] in run._SEQUENCE_SCRIPTS:
        for row in SET_SCORES:
            if getattr(a, row.name) and row.sequences is not True:
                ap.error('--%s: %s' % (row.name, row.sequences))
        if a.probe or a.probe_wide:
            ap.error('--probe: %s' % _NO_CODE)
        if a.frechet:
            ap.error('--frechet: %s' % _NO_CODE)
        if a.swd:
            ap.error('--swd: %s' % _NO_CODE)
        if a.cls:
            ap.error('--cls: the state-space scripts have no single set of images to classify')
        if a.kmeans:
            ap.error('--kmeans: the state-space scripts have no single set of images to bin')
    if a.manifold:          # (checked before anything is built)
        name = os.path.splitext(os.path.basename(a.script))[0]
        if name not in MANIFOLD_SCRIPTS:
            ap.error('--manifold: the latent-space pictures exist for %s only, not for %s' % (' and '.join(MANIFOLD_SCRIPTS), name))
        if not a.out_dir:
            ap.error('--manifold writes pictures: it needs --out-dir')
    S = run.reference_block(a.script, **over)
    S.update(DATA_DIR=a.data_dir, SCRIPT=a.script)
    cfg, model = run.config(S), None
    if S['DATASET'] in run.SEQUENCE_DATASETS:
        from .models_ssgan import StateSpaceGAN
        if not a.out_dir and not any(getattr(a, row.name) for row in SET_SCORES):
            ap.error('--out-dir is required for %s: its passes are files' % a.script)
        model = StateSpaceGAN(cfg)
    ema = None
    if a.ema:
        try:
            ema = checkpoint.ema_params(a.ckpt)
        except ValueError as e:
            ap.error('--ema: %s' % e)
    tr = Trainer(cfg, device=lib.get_device(), graph=False, model=model)
    checkpoint.restore(a.ckpt, tr)
    if a.ema:
        # no optimizer is built here, so there is no average to visit: the averaged values ARE this process's weights (the critic's stay
        # the checkpoint's live ones), and the evaluators only name what they write
        tr.load_params(ema)
        tr.ema_loaded = True
    res = evaluate_once(tr, S, out_dir=a.out_dir, manifold=a.manifold, probe=a.probe or a.probe_wide, probe_wide=a.probe_wide, frechet=a.frechet, swd=a.swd, cls=a.cls, kmeans=a.kmeans, **{row.name: getattr(a, row.name) for row in SET_SCORES})
    for k in sorted(res):
        print('%s\t%s' % (k, res[k]))
    return res


def evaluate_once(tr, S, out_dir=None, frame='eval', manifold=False, probe=False, probe_wide=False, frechet=False, swd=False, cls=False, kmeans=False, **scores):
    """every pass the script's data allow, once -> {name: value}; manifold: the latent-space pictures too (labelled dev data only);
    probe: the three values of Evaluator.probe_scores too, after the set-level scores (image scripts; skipped with one message where the
    dev set or the training split has no labels); probe_wide: implies probe, and the four values of PROBE_WIDE_KEYS after its three; frechet: the four values of Evaluator.frechet_scores too, after those (image scripts; no
    labels needed); swd: the four values of Evaluator.swd_scores too, after those (image scripts; no labels needed); cls: the five values of
    Evaluator.classifier_scores too, after those (image scripts; skipped with one message where the dev set or the training split has no labels);
    kmeans: the values of Evaluator.kmeans_scores too, after those (image scripts; the two z rows need a labelled dev set);
    scores: the set-level scores of SET_SCORES to add, by name (mmd=True, ...: Evaluator.set_scores' keywords, one build of the sets for all
    of them; a score that needs labels is skipped on unlabelled dev data); a trainer whose weights are averaged ones loaded from a
    checkpoint (tr.ema_loaded, main --ema): names and files carry the suffixes.  The state-space scripts: the video files (with out_dir)
    and, with rec, the four reconstruction values of the dev sequences' frames"""
    _known('evaluate_once', scores)
    from . import run
    ema_names = bool(getattr(tr, 'ema_loaded', False))
    if S['DATASET'] in run.SEQUENCE_DATASETS:       # the video passes: files only (train_data: the first dev minibatch)
        if probe or probe_wide:
            raise ValueError('probe: %s' % _NO_CODE)
        if frechet:
            raise ValueError('frechet: %s' % _NO_CODE)
        if swd:
            raise ValueError('swd: %s' % _NO_CODE)
        if cls:
            raise ValueError('cls: the state-space scripts have no single set of images to classify')
        if kmeans:
            raise ValueError('kmeans: the state-space scripts have no single set of images to bin')
        ev = SequenceEvaluator(tr, S)
        ev.weights = 'ema' if ema_names else 'live'
        dev, _ = run.eval_sets(S, tr.model, tr.device)
        res = {}
        if scores.get('rec'):
            res.update(ev.tag(ev.rec_scores(run.rec_sequences(S, tr.model, tr.device))))
        if out_dir:
            ev.set_fixed_data(dev[0])
            os.makedirs(out_dir, exist_ok=True)
            res['files'] = ' '.join(os.path.basename(p) for p in ev.save_videos(out_dir, frame, train_data=dev[0]))
        return res
    ev = Evaluator(tr, S)
    ev.weights = 'ema' if ema_names else 'live'
    dev, test = run.eval_sets(S, tr.model, tr.device)
    res = dict(ev.tag(ev.dev_costs(dev)))
    if tr.cfg.K and test is not None:
        res.update(ev.tag({'testing accuracy': ev.cluster_accuracy(test)}))
    for row in SET_SCORES:
        if scores.get(row.name) and 'labels' in row.needs and not run.labelled(dev):
            print('[evaluate] %s skipped: no labelled dev set' % row.title)
            scores[row.name] = False
    if any(scores.values()):
        res.update(ev.tag(ev.set_scores(dev, **scores)))
    if probe or probe_wide:
        fit = run.probe_sets(S) if run.labelled(dev) else None
        if not fit:
            print('[evaluate] dev probe accuracy skipped: no labelled dev set and training split')
        else:
            res.update(ev.tag(ev.probe_scores(fit, dev, wide=probe_wide)))
    if frechet:
        res.update(ev.tag(ev.frechet_scores(dev)))
    if swd:
        res.update(ev.tag(ev.swd_scores(dev)))
    if cls:
        fit = run.classifier_sets(S) if run.labelled(dev) else None
        if not fit:
            print('[evaluate] dev classifier score skipped: no labelled dev set and training split')
        else:
            res.update(ev.tag(ev.classifier_scores(fit, dev)))
    if kmeans:
        res.update(ev.tag(ev.kmeans_scores(run.kmeans_sets(S, tr.model, tr.device), dev)))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        ev.set_fixed_data(dev[0])
        ev.save_images(out_dir, frame)
    if manifold:
        if not run.labelled(dev):
            print('[evaluate] latent-space t-SNE skipped: no labelled dev set')
        else:
            res['manifold files'] = ' '.join(os.path.basename(p) for p in ev.manifold(dev, out_dir, frame))
    return res


if __name__ == '__main__':
    main()
