"""Wall time of Evaluator.swd_scores at a script's defaults and 10000 rows, next to the `dev frechet` pass at the same rows, the share of the
swd_* kernels, and the op against the plain torch composition (sort, subtract, square, mean) on arrays of the pass's size (docs/KERNELS.md,
the sliced-Wasserstein section).  Synthetic images and a randomly initialised model: timing only.
`python tools/swd_time.py [script]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from graphical_gan_amd import run, _lib, functional as F  # noqa: E402
from graphical_gan_amd import tflib as lib  # noqa: E402
from graphical_gan_amd.engine import Trainer  # noqa: E402
from graphical_gan_amd.evaluate import Evaluator, SWD_MAX_ROWS, SWD_DIRS  # noqa: E402


def torch_composition(px, py):
    """what a user of torch has instead, equal sizes and p = 2: (sqrt(mean_l), sqrt(max_l)) of mean_i (sort(px) - sort(py))^2"""
    d = torch.sort(px, dim=0).values.double() - torch.sort(py, dim=0).values.double()
    per = (d * d).mean(dim=0)
    return torch.stack([per.mean().sqrt(), per.max().sqrt()])


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps, out


def main(script='gan_inference_cifar10'):
    S = run.reference_block(script)
    S.update(SYNTHETIC='force')
    cfg = run.config(S)
    tr = Trainer(cfg, device=lib.get_device(), graph=False)
    B, D = S['BATCH_SIZE'], cfg.output_dim
    rng = np.random.default_rng(0)
    mk = (lambda: rng.random((B, D), dtype=np.float32)) if cfg.dataset == 'mnist' else (lambda: rng.integers(0, 256, size=(B, D)).astype(np.int32))
    dev = [mk() for _ in range(SWD_MAX_ROWS // B)]
    ev = Evaluator(tr, S)
    print('%s: DIM_LATENT %d, %d pixel columns, minibatches of %d, %d dev rows, %d directions' % (script, cfg.dim_latent, D, B, len(dev) * B, SWD_DIRS))
    L = _lib.load()
    for rep in range(4):
        if rep == 3:
            L.ggan_prof_reset()
            L.ggan_prof_enable(1)
        torch.cuda.synchronize()
        t0 = time.time()
        res = ev.swd_scores(dev)
        torch.cuda.synchronize()
        print('swd pass %d%s: last_seconds %.3f, wall %.3f, %s' % (rep, ' (warm-up)' if rep == 0 else ' (kernel timers on)' if rep == 3 else '', ev.last_seconds, time.time() - t0, res))
    L.ggan_prof_enable(0)
    for r in sorted(_lib.prof_report(), key=lambda r: -r['total_ms']):
        if r['name'].startswith('swd'):
            print('%-24s %8.3f ms in %d launches' % (r['name'], r['total_ms'], r['launches']))
    L.ggan_prof_reset()
    for rep in range(3):
        res = ev.frechet_scores(dev)
        print('for comparison, dev frechet over the same rows, pass %d: last_seconds %.3f, %s' % (rep, ev.last_seconds, res))
    # the op against the torch composition on arrays of the pass's size, alternating in one process, device events after warm-up
    rows = len(dev) * B
    g = torch.Generator(device='cpu').manual_seed(0)
    px = torch.randn((rows, SWD_DIRS), generator=g).to(tr.device)
    py = (1.1 * torch.randn((rows, SWD_DIRS), generator=g) + 0.1).to(tr.device)
    op = lambda: F.sliced_wasserstein_projected(px, py, 2)[0]
    ref = lambda: torch_composition(px, py)
    timed(op, 3)
    timed(ref, 3)
    for rep in range(3):
        t_op, v = timed(op, 10)
        t_ref, w = timed(ref, 10)
        print('[%d, %d] pass %d: the op %.3f ms, torch sort + subtract + square + mean %.3f ms; values %s against %s'
              % (rows, SWD_DIRS, rep, t_op, t_ref, v.cpu().numpy(), w.cpu().numpy()))


if __name__ == '__main__':
    main(*sys.argv[1:2])
