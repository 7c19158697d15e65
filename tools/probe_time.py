"""Wall time of Evaluator.probe_scores at a script's defaults, and the share of the probe's own kernels (docs/KERNELS.md, the probe section).
Synthetic labelled images and a randomly initialised model: timing only.  `python tools/probe_time.py [script]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from graphical_gan_amd import run, _lib  # noqa: E402
from graphical_gan_amd import tflib as lib  # noqa: E402
from graphical_gan_amd.engine import Trainer  # noqa: E402
from graphical_gan_amd.evaluate import Evaluator, PROBE_FIT_ROWS, PROBE_MAX_ROWS  # noqa: E402


def main(script='gan_inference_cifar10'):
    S = run.reference_block(script)
    S.update(SYNTHETIC='force')
    cfg = run.config(S)
    tr = Trainer(cfg, device=lib.get_device(), graph=False)
    B, D = S['BATCH_SIZE'], cfg.output_dim
    rng = np.random.default_rng(0)
    proto = rng.integers(0, 256, size=(10, D))

    def batches(n):
        out = []
        for _ in range(n):
            y = rng.integers(0, 10, size=B)
            x = np.clip(0.5 * proto[y] + 0.5 * rng.integers(0, 256, size=(B, D)), 0, 255)
            out.append(((x / 255.0).astype(np.float32) if cfg.dataset == 'mnist' else x.astype(np.int32), y.astype(np.int64)))
        return out
    fit, dev = batches(PROBE_FIT_ROWS // B), batches(PROBE_MAX_ROWS // B)
    ev = Evaluator(tr, S)
    print('%s: DIM_LATENT %d, minibatches of %d, %d fit rows, %d dev rows' % (script, cfg.dim_latent, B, len(fit) * B, len(dev) * B))
    L = _lib.load()
    for rep in range(3):
        if rep == 2:
            L.ggan_prof_reset()
            L.ggan_prof_enable(1)
        torch.cuda.synchronize()
        t0 = time.time()
        res = ev.probe_scores(fit, dev)
        torch.cuda.synchronize()
        print('pass %d: last_seconds %.3f, wall %.3f, %s' % (rep, ev.last_seconds, time.time() - t0, res))
    L.ggan_prof_enable(0)
    for r in sorted(_lib.prof_report(), key=lambda r: -r['total_ms']):
        if r['name'].startswith('probe'):
            print('%-24s %8.3f ms in %d launches' % (r['name'], r['total_ms'], r['launches']))
    L.ggan_prof_reset()
    ev.set_scores(dev, knn=True)
    print('for comparison, dev knn accuracy over the dev rows: last_seconds %.3f' % ev.last_seconds)


if __name__ == '__main__':
    main(*sys.argv[1:2])
