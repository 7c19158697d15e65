"""Counterpart of the reference's gmgan_inference_face.py for this package's tflib: the same UPPERCASE hyper-parameter block
(gmgan_inference_face.py:35-54; `run.reference_block` holds it as data and derives the MODE-dependent constants as the script does), nets and
step order; runs on one MI355X.  `python scripts/gmgan_inference_face.py [ITERS]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphical_gan_amd import run

MODE = 'local_ep'  # ali, local_ep
SETTINGS = run.reference_block(__file__, MODE=MODE)
# edit the block here, e.g. SETTINGS['N_COMS'] = 10 -- or pass it to reference_block, which then derives N_VIS etc. from it
SETTINGS.update(DATA_DIR=os.environ.get('GGAN_DATA_DIR', ''), OUT_DIR=os.environ.get('GGAN_OUT_DIR', ''), SAVE_EVERY=10000, LOG_EVERY=100)
SETTINGS.update(run.eval_settings(__file__))     # dev costs / samples / reconstructions (/ testing accuracy) at the reference's cadence
SETTINGS.update(run.score_settings(__file__))   # the set-level dev scores, off when unset: every $GGAN_MMD_EVERY / $GGAN_PRDC_EVERY / $GGAN_KNN_EVERY / $GGAN_PARZEN_EVERY / $GGAN_REC_EVERY iterations
SETTINGS.update(run.probe_settings(__file__))   # the least-squares linear probe of the codes, off when unset: dev / fit probe accuracy z and dev probe accuracy xr every $GGAN_PROBE_EVERY iterations
SETTINGS.update(run.frechet_settings(__file__))   # the Frechet distance of codes and of projected images, off when unset: dev frechet z / xr and their mean parts every $GGAN_FRECHET_EVERY iterations
SETTINGS.update(run.swd_settings(__file__))   # the sliced Wasserstein distance of codes and of images in the full pixel space, off when unset: dev swd z / x and their max rows every $GGAN_SWD_EVERY iterations
SETTINGS.update(run.classifier_settings(__file__))   # the classifier score of generated images, off when unset: dev classifier score x / score std x / score data / accuracy / frechet x every $GGAN_CLS_EVERY iterations (labelled data only)
SETTINGS.update(run.kmeans_settings(__file__))   # NDB of the generated images and k-means clustering scores of the codes, off when unset: dev ndb x / ndb js x / ndb data / kmeans accuracy z / kmeans nmi z every $GGAN_KMEANS_EVERY iterations (the z rows: labelled data only)
SETTINGS.update(run.ema_settings(__file__))      # $GGAN_EMA_DECAY: average the generator-side weights; $GGAN_EMA_EVAL = live | ema | both: which the passes score
if len(sys.argv) > 1:
    SETTINGS['ITERS'] = int(sys.argv[1])
globals().update(SETTINGS)          # BATCH_SIZE, DIM, DIM_LATENT, CRITIC_ITERS, ... as module constants, as in the reference
run.train(SETTINGS, run.config(SETTINGS))
