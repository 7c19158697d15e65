"""Time of one iteration of gmgan_inference_cifar10 (N_COMS 30, 64 images) in each MODE on an MI355X, for docs/KERNELS.md.

  python tools/gmgan_modes_time.py [--modes local_ep,ali,alice,vegan,local_ep] [--steps 200] [--warmup 20] [--repeats 5]

Each MODE is built the way bench.py builds its gmgan row: engine.Trainer with step graphs, the device-resident ring of synthetic
minibatches, one graph replay per iteration (1 generator step + CRITIC_ITERS critic steps: 1, under vegan 5).  Timed like bench.py: a
host clock around `--steps` iterations between two device synchronisations, `--repeats` windows per MODE; median, min and max of the
per-iteration milliseconds.  The MODEs run one after the other in one process; local_ep, the existing path, is by default timed first AND
last, so that the spread between its two blocks stands beside the differences between the MODEs.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_mode(mode, a, dev):
    import torch
    from graphical_gan_amd import tflib as lib, optim
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models import Config
    optim.reset_optimizers()
    lib.delete_all_params()
    np.random.seed(0)
    thin = mode == 'vegan'                         # (gmgan_inference_cifar10.py:72-77: DIM_LATENT 8, no BatchNorm)
    cfg = Config('cifar10', batch_size=64, n_coms=30, mode=mode, dim_latent=8 if thin else 128, bn=False if thin else None)
    tr = Trainer(cfg, device=dev, graph=True, seed=1234)
    ring = tr.model.synthetic_ring(dev, n=8, seed=1234)

    def batches():
        i = 0
        while True:
            yield ring[i % len(ring)]
            i += 1
    bi, it = batches(), 0
    for _ in range(2):
        tr.iteration(it, bi); it += 1
    tr.use_ring(ring)
    for _ in range(max(a.warmup, 2)):
        tr.iteration(it, bi); it += 1
    tr.flush()
    torch.cuda.synchronize(dev)
    windows, last = [], None
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            last = tr.iteration(it, bi); it += 1
        tr.flush()
        torch.cuda.synchronize(dev)
        windows.append(1e3 * (time.perf_counter() - t0) / a.steps)
    return dict(mode=mode, critic=cfg.critic, critic_iters=cfg.critic_iters, dim_latent=cfg.dim_latent,
                ms_per_iteration=dict(median=float(np.median(windows)), min=float(min(windows)), max=float(max(windows)), windows=windows),
                finite=bool(all(np.isfinite(float(v)) for v in last.values())), one_graph_per_iteration=tr._iter_graph is not None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--modes', default='local_ep,ali,alice,vegan,local_ep')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for mode in a.modes.split(','):
        rows.append(time_mode(mode, a, dev))
        print('[gmgan_modes_time] %-9s %.4f ms / iteration (min %.4f, max %.4f)' % (
            mode, rows[-1]['ms_per_iteration']['median'], rows[-1]['ms_per_iteration']['min'], rows[-1]['ms_per_iteration']['max']), flush=True)
    print(json.dumps(dict(workload='gmgan_inference_cifar10 N_COMS 30 bs 64, ring, one graph per iteration', steps=a.steps, rows=rows)))


if __name__ == '__main__':
    main()
