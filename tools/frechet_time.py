"""Wall time of Evaluator.frechet_scores at a script's defaults and 10000 rows, next to the `dev mmd` pass at the same rows, and the share of
the Frechet kernels (docs/KERNELS.md, the Frechet section).  Synthetic images and a randomly initialised model: timing only.
`python tools/frechet_time.py [script]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from graphical_gan_amd import run, _lib  # noqa: E402
from graphical_gan_amd import tflib as lib  # noqa: E402
from graphical_gan_amd.engine import Trainer  # noqa: E402
from graphical_gan_amd.evaluate import Evaluator, FRECHET_MAX_ROWS  # noqa: E402


def main(script='gan_inference_cifar10'):
    S = run.reference_block(script)
    S.update(SYNTHETIC='force')
    cfg = run.config(S)
    tr = Trainer(cfg, device=lib.get_device(), graph=False)
    B, D = S['BATCH_SIZE'], cfg.output_dim
    rng = np.random.default_rng(0)
    mk = (lambda: rng.random((B, D), dtype=np.float32)) if cfg.dataset == 'mnist' else (lambda: rng.integers(0, 256, size=(B, D)).astype(np.int32))
    dev = [mk() for _ in range(FRECHET_MAX_ROWS // B)]
    ev = Evaluator(tr, S)
    print('%s: DIM_LATENT %d, minibatches of %d, %d dev rows' % (script, cfg.dim_latent, B, len(dev) * B))
    L = _lib.load()
    for rep in range(3):
        if rep == 2:
            L.ggan_prof_reset()
            L.ggan_prof_enable(1)
        torch.cuda.synchronize()
        t0 = time.time()
        res = ev.frechet_scores(dev)
        torch.cuda.synchronize()
        print('frechet pass %d: last_seconds %.3f, wall %.3f, %s' % (rep, ev.last_seconds, time.time() - t0, res))
    L.ggan_prof_enable(0)
    for r in sorted(_lib.prof_report(), key=lambda r: -r['total_ms']):
        if r['name'].startswith('frechet'):
            print('%-24s %8.3f ms in %d launches' % (r['name'], r['total_ms'], r['launches']))
    L.ggan_prof_reset()
    for rep in range(2):
        res = ev.set_scores(dev, mmd=True)
        print('for comparison, dev mmd over the same rows, pass %d: last_seconds %.3f, %s' % (rep, ev.last_seconds, res))


if __name__ == '__main__':
    main(*sys.argv[1:2])
