"""Time of the Parzen-window ops (functional.parzen_lse / parzen_ll, csrc/parzen_sets.hip) on an MI355X, for docs/KERNELS.md.

  python tools/parzen_time.py [--n 10000] [--ns 10] [--dims 784 3072] [--repeat 7] [--calls 10] [--chunk 2048]

Per width d: two sets of n image-like rows, and three ways over them, every one warmed twice and then timed in `--repeat` rounds that
ALTERNATE the three (a window of `--calls` back-to-back calls between two HIP events each; per-call median, min and max printed):
  parzen_ll      the pass's one call: all rows, `--ns` bandwidths of logspace(-1, 0), one sweep of Gram tiles, the final combination;
  torch          what a user of torch would write: squared Gram-form distances in row chunks of `--chunk` (`torch.cdist`), and one
                 `torch.logsumexp` per bandwidth and chunk;
  knn_accuracy   the k-NN pass's sweep over n rows of the same width against themselves (k = 5): the yardstick of the Gram work.
The two log-likelihoods are compared.  FLOP: the launches' own count (tiles computed x 2 x 128 x 128 x d) over the time, against the
fp32-MFMA peak of 157.3 TFLOP/s; libggan's per-kernel timers give every kernel's time alone.  One JSON line at the end."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3
KERNELS = ('parzen_norms', 'parzen_lse', 'parzen_final', 'knn_lists')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--ns', type=int, default=10)
    ap.add_argument('--dims', type=int, nargs='+', default=[784, 3072])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--chunk', type=int, default=2048)
    a = ap.parse_args()
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    sig = [float(v) for v in np.logspace(-1, 0, a.ns)]

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def torch_ll(x, gx):
        n, d = gx.shape
        out = torch.empty((len(sig), x.shape[0]), dtype=torch.float64, device=dev)
        for r0 in range(0, x.shape[0], a.chunk):
            D = torch.cdist(x[r0:r0 + a.chunk], gx, compute_mode='use_mm_for_euclid_dist') ** 2
            for g, s in enumerate(sig):
                out[g, r0:r0 + a.chunk] = torch.logsumexp(D * (-0.5 / (s * s)), dim=1).double() - (math.log(n) + 0.5 * d * math.log(2 * math.pi * s * s))
        return out

    out, L = {}, _lib.load()
    for d in a.dims:
        g = torch.Generator(device=dev)
        g.manual_seed(d)
        x, gx = torch.rand(a.n, d, device=dev, generator=g) ** 3, torch.rand(a.n, d, device=dev, generator=g) ** 3     # pixels in [0, 1)
        y = torch.randint(0, 10, (a.n,), device=dev, generator=g).int()
        ways = dict(parzen_ll=lambda: F.parzen_ll(x, gx, sig), torch=lambda: torch_ll(x, gx), knn_accuracy=lambda: F.knn_accuracy(x, y, 5))
        ours, ref = ways['parzen_ll'](), ways['torch']()
        rec = dict(max_rel_diff_to_torch=float(((ours - ref).abs() / ref.abs().clamp(min=1.0)).max().item()), ll_min=float(ours.min().item()))
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
        for _ in range(3):
            ways['parzen_ll'](); ways['knn_accuracy']()
        torch.cuda.synchronize()
        rep = {r['name']: r for r in _lib.prof_report() if r['name'] in KERNELS}
        L.ggan_prof_enable(0)
        rec['kernels_ms'] = {name: r['total_ms'] / r['launches'] for name, r in rep.items()}
        for name in ('parzen_lse', 'knn_lists'):
            rec['tflops_' + name] = rep[name]['flops'] / rep[name]['launches'] / (rec['kernels_ms'][name] * 1e-3) / 1e12
            rec['of_fp32_mfma_peak_' + name] = rec['tflops_' + name] / PEAK_TFLOPS
        out['d%d' % d] = rec
        print('d = %d: %s' % (d, json.dumps(rec)))
        del x, gx
    print(json.dumps(out))


if __name__ == '__main__':
    main()
