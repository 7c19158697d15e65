"""Counterpart of the reference's ssgan_inference_chairs.py for this package's tflib: the same UPPERCASE hyper-parameter block
(ssgan_inference_chairs.py:28-57; `run.reference_block` holds it as data and derives the MODE-dependent constants as the script does), nets and
step order; runs on one MI355X.  `python scripts/ssgan_inference_chairs.py [ITERS]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphical_gan_amd import run

MODE = 'local_ep'  # local_ep, local_epce-z, ali, alice-z (ALI_MODE concat_x | concat_z | 3dcnn; POS_MODE, OP_DYN_MODE: see the block)
BN_FLAG = False  # BatchNorm in the frame generator, extractors and critics (BN_FLAG_G / _E / _D follow it; see the block)
SETTINGS = run.reference_block(__file__, MODE=MODE, BN_FLAG=BN_FLAG)
# edit the block here, e.g. SETTINGS['N_COMS'] = 10 -- or pass it to reference_block, which then derives N_VIS etc. from it
SETTINGS.update(run.eval_settings(__file__))  # the video passes every 5000 iterations: samples / train_data / reconstruction / disentangle
SETTINGS.update(run.score_settings(__file__))   # the set-level dev scores, off when unset: dev rec mse / psnr / ssim / ssim se x every $GGAN_REC_EVERY iterations (the other four are the image scripts')
SETTINGS.update(run.ema_settings(__file__))      # $GGAN_EMA_DECAY: average the generator-side weights; $GGAN_EMA_EVAL = live | ema | both: which the passes score
SETTINGS.update(DATA_DIR=os.environ.get('GGAN_DATA_DIR', ''), OUT_DIR=os.environ.get('GGAN_OUT_DIR', ''), SAVE_EVERY=10000, LOG_EVERY=100)
if len(sys.argv) > 1:
    SETTINGS['ITERS'] = int(sys.argv[1])
globals().update(SETTINGS)          # BATCH_SIZE, DIM, DIM_LATENT, CRITIC_ITERS, ... as module constants, as in the reference
from graphical_gan_amd.models_ssgan import StateSpaceGAN
cfg = run.config(SETTINGS)
run.train(SETTINGS, cfg, model=StateSpaceGAN(cfg))
