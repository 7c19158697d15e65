"""Time of the reconstruction-fidelity op (functional.ssim_pairs, csrc/ssim_pairs.hip) and of the dev-set passes on it, on an MI355X, for
docs/KERNELS.md.

  python tools/rec_time.py [--repeat 7] [--calls 10] [--no-pass]

Two shapes: 10000 x 3 x 32 x 32 (the image scripts' pass at its row cap, CIFAR planes) and 512 x 1 x 64 x 64 (one moving-MNIST minibatch
of 32 sequences of 16 frames: the largest LDS footprint).  Per shape, on image-like rows against a noisy copy:
  ssim_pairs     the op alone: both launches, a window of `--calls` back-to-back calls between two HIP events, `--repeat` windows; per-call
                 median, min and max;
  torch          what a user of torch would write: five grouped separable convolutions (x, y, xx, yy, xy) and the map, alternated with
                 the op window by window; the two results are compared;
  kernels        libggan's per-kernel timers: ssim_planes and ssim_images alone, and the bytes-moved bound 2 n c h w 4 bytes over the
                 measured HBM rate of 6.29 TB/s;
  pass           (unless --no-pass) the whole pass, nets included, wall clock with a device synchronisation on both sides: at the first
                 shape Evaluator.rec_scores of a randomly initialised gan_inference_cifar10 model over 156 synthetic minibatches of 64, at
                 the second SequenceEvaluator.rec_scores of a randomly initialised ssgan_inference_moving_mnist model (BATCH_SIZE 32, N_C 8) over one.
One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29          # measured float4 copy rate (8.0 TB/s spec)
SHAPES = [(10000, 3, 32, 32), (512, 1, 64, 64)]
KERNELS = ('ssim_planes', 'ssim_images')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--no-pass', action='store_true')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    from graphical_gan_amd import functional as F, _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    k = torch.arange(11, dtype=torch.float64, device=dev) - 5
    g = torch.exp(-0.5 * k * k / 2.25)
    g = (g / g.sum()).float()

    def torch_ssim(x, y, shape):
        c, h, w = shape
        x, y = x.view(-1, c, h, w), y.view(-1, c, h, w)
        kh, kv = g.view(1, 1, 1, 11).repeat(c, 1, 1, 1), g.view(1, 1, 11, 1).repeat(c, 1, 1, 1)
        blur = lambda v: TF.conv2d(TF.conv2d(v, kh, groups=c), kv, groups=c)
        mx, my = blur(x), blur(y)
        sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        m = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
        return ((x - y) ** 2).mean(dim=(1, 2, 3)), m.mean(dim=(1, 2, 3))

    out, L = {}, _lib.load()
    for n, c, h, w in SHAPES:
        shape = (c, h, w)
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        x = torch.rand(n, c * h * w, device=dev, generator=gen) ** 3                    # pixels in [0, 1)
        y = (x + 0.05 * torch.randn(n, c * h * w, device=dev, generator=gen)).clamp_(0, 1)
        ways = dict(ssim_pairs=lambda: F.ssim_pairs(x, y, shape), torch=lambda: torch_ssim(x, y, shape))
        ours, ref = ways['ssim_pairs'](), ways['torch']()
        rec = dict(max_abs_diff_to_torch_mse=float((ours[0] - ref[0]).abs().max().item()),
                   max_abs_diff_to_torch_ssim=float((ours[1] - ref[1]).abs().max().item()), ssim_mean=float(ours[1].mean().item()))
        for fn in ways.values():
            fn(); fn()
        torch.cuda.synchronize()
        times = {name: [] for name in ways}
        for _ in range(a.repeat):
            for name, fn in ways.items():
                times[name].append(window(fn))
        for name, ts in times.items():
            rec[name] = dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))
        L.ggan_prof_reset(); L.ggan_prof_enable(1)
        for _ in range(5):
            ways['ssim_pairs']()
        torch.cuda.synchronize()
        rep = {r['name']: r for r in _lib.prof_report() if r['name'] in KERNELS}
        L.ggan_prof_enable(0)
        rec['kernels_ms'] = {name: r['total_ms'] / r['launches'] for name, r in rep.items()}
        nbytes = 2.0 * n * c * h * w * 4
        rec['bytes_moved'] = nbytes
        rec['bound_ms'] = nbytes / (HBM_TBS * 1e12) * 1e3
        rec['of_hbm_rate_ssim_planes'] = rec['bound_ms'] / rec['kernels_ms']['ssim_planes']
        out['%dx%dx%dx%d' % (n, c, h, w)] = rec
        print('%s: %s' % ((n, c, h, w), json.dumps(rec)))
        del x, y
    if not a.no_pass:
        out['pass'] = passes(dev)
        print('pass: %s' % json.dumps(out['pass']))
    print(json.dumps(out))


def passes(dev, rounds=5):
    """wall time of the two passes, nets included: median of `rounds` after one warm-up"""
    import torch
    from graphical_gan_amd import run
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd import optim
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.evaluate import Evaluator, SequenceEvaluator
    from graphical_gan_amd.models_ssgan import StateSpaceGAN

    def timed(fn):
        fn()
        ts = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.time()
            res = fn()
            torch.cuda.synchronize()
            ts.append((time.time() - t0) * 1e3)
        return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), values=res)

    out = {}
    S = run.reference_block('gan_inference_cifar10', SYNTHETIC='force')
    tr = Trainer(run.config(S), device=dev, graph=False)
    dev_set = tr.model.synthetic_ring(dev, n=157, seed=4321)
    ev = Evaluator(tr, S)
    out['gan_inference_cifar10 156 x 64 images'] = timed(lambda: ev.rec_scores(dev_set))
    # the nets' share: the same build of the sets without the scoring
    def sets_only():
        with ev._guard():
            ev._score_sets(dev_set, 10000, generated=False, rec=True)
    out['gan_inference_cifar10 156 x 64 images']['sets_alone_median_ms'] = timed(lambda: sets_only())['median_ms']
    del tr, ev, dev_set
    optim.reset_optimizers()
    lib.delete_all_params()
    S = run.reference_block('ssgan_inference_moving_mnist', SYNTHETIC='force', BATCH_SIZE=32, N_C=8)
    cfg = run.config(S)
    tr = Trainer(cfg, device=dev, graph=False, model=StateSpaceGAN(cfg))
    seqs = run.rec_sequences(S, tr.model, dev)[:1]
    sev = SequenceEvaluator(tr, S)
    out['ssgan_inference_moving_mnist 32 x 16 frames'] = timed(lambda: sev.rec_scores(seqs))
    out['ssgan_inference_moving_mnist 32 x 16 frames']['reconstructions_alone_median_ms'] = timed(lambda: (sev.reconstructions(seqs[0]), None)[1])['median_ms']
    return out


if __name__ == '__main__':
    main()
