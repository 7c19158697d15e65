"""Cost of the evaluation-only weight average (csrc/optim.hip: ema_k, swap_k) on an MI355X, for docs/KERNELS.md.

  python tools/ema_time.py [--decay 0.999 | --decay off] [--steps 200] [--warmup 20] [--repeats 5] [--no-kernels]

The headline workload of bench.py -- gan_inference_cifar10, MODE wali-gp, 64 images, the device-resident ring, one graph replay per
iteration of 1 generator + 5 critic steps -- built the way bench.py builds it, with engine.Trainer's ema_decay set (or, --decay off,
without it: the same driver's own baseline, to be alternated with the averaging run and set beside `python bench.py` of the parent
commit).  Timed like bench.py: a host clock around `--steps` iterations between two device synchronisations, `--repeats` windows;
median, min and max of the per-iteration milliseconds.
Unless --no-kernels, the two kernels alone on buffers of the generator-side optimizer's size: windows of 20 back-to-back launches
between two HIP events, per-launch median, with the bytes they move (12 B / 16 B per element) over that time.  For the kernel's time
INSIDE the step, run this under `rocprofv3 --kernel-trace --stats -- python tools/ema_time.py --no-kernels --steps 100 --repeats 1`
and read ema_k's row (one launch per generator step: those of the eager, warm-up and capture iterations are in its count).
One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--decay', default='0.999')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-kernels', action='store_true')
    a = ap.parse_args()
    import torch
    from graphical_gan_amd import functional as F, optim
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models import Config
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    decay = None if a.decay == 'off' else float(a.decay)
    np.random.seed(0)
    cfg = Config('cifar10', batch_size=64, n_coms=0, mode='wali-gp')
    tr = Trainer(cfg, device=dev, graph=True, seed=1234, ema_decay=decay)
    torch.manual_seed(1234)
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
    gen = next(o for key, o in optim._optimizers.items() if key[0] == 'gen')
    out = dict(workload='gan_inference_cifar10 wali-gp bs 64, ring, one graph per iteration', ema_decay=decay, steps=a.steps,
               ms_per_iteration=dict(median=float(np.median(windows)), min=float(min(windows)), max=float(max(windows)), windows=windows),
               finite=bool(all(np.isfinite(float(v)) for v in last.values())), one_graph_per_iteration=tr._iter_graph is not None,
               gen_params=int(sum(p.numel() for p in gen.params)), gen_flat_floats=int(gen.total), shadow=gen.shadow is not None)
    if not a.no_kernels:
        n = int(gen.total)
        x, y = torch.randn(n, device=dev), torch.randn(n, device=dev)
        step = torch.full((1,), 12345, dtype=torch.int32, device=dev)

        def window(fn, calls=20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / calls
        for name, fn, bpe in (('ema_step', lambda: F.ema_step_(x, y, step, 0.999), 12.0), ('swap', lambda: F.swap_(x, y), 16.0)):
            fn(); fn()
            torch.cuda.synchronize(dev)
            ts = [window(fn) for _ in range(7)]
            ms = float(np.median(ts))
            out[name] = dict(n=n, median_us=1e3 * ms, min_us=1e3 * float(min(ts)), max_us=1e3 * float(max(ts)), bytes=bpe * n,
                             tb_per_s=bpe * n / (ms * 1e-3) / 1e12)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
