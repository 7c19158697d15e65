"""Time of the labelled neighbour-list ops (functional.knn_lists / knn_vote / knn_accuracy, csrc/knn_lists.hip) on an MI355X, for docs/KERNELS.md.

  python tools/knn_time.py [--n 10000] [--k 5] [--dims 128 3072] [--repeat 7] [--calls 10] [--chunk 2048] [--classes 10]

Per width d: a labelled set of n rows, and three ways over it, every one warmed twice and then timed in `--repeat` rounds that ALTERNATE
the three (a window of `--calls` back-to-back calls between two HIP events each; per-call median, min and max of the windows printed):
  knn_accuracy   the leave-one-out accuracy: one index-list sweep, the final merge, the vote;
  torch          what a user of torch would write: Gram-form distances in row chunks of `--chunk` (`torch.cdist`, so that no n x n matrix is
                 held), own index set to +inf, `topk(k, largest=False)` per chunk, the labels gathered and `torch.mode` along the list;
  knn_radii      the same sweep WITHOUT indices (csrc/knn_sets.hip, unchanged): the yardstick for what carrying the indices costs.
The two accuracies are compared (they may differ in rows whose k-th and k+1-th distances tie to float32 rounding, and torch.mode breaks a
tied vote its own way).  FLOP: the launches' own count (tiles computed x 2 x 128 x 128 x d) over the time, against the fp32-MFMA peak of
157.3 TFLOP/s; libggan's per-kernel timers give every kernel's time alone.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3
KERNELS = ('knn_lists_norms', 'knn_lists', 'knn_lists_final', 'knn_vote', 'knn_norms', 'knn_radii', 'knn_final')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--dims', type=int, nargs='+', default=[128, 3072])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--classes', type=int, default=10)
    a = ap.parse_args()
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    k = a.k

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def torch_accuracy(z, y):
        hits = torch.zeros((), dtype=torch.int64, device=dev)
        for r0 in range(0, z.shape[0], a.chunk):
            D = torch.cdist(z[r0:r0 + a.chunk], z, compute_mode='use_mm_for_euclid_dist')
            i = torch.arange(D.shape[0], device=dev)
            D[i, i + r0] = float('inf')
            idx = D.topk(k, dim=1, largest=False).indices
            pred = torch.mode(y[idx], dim=1).values
            hits += (pred == y[r0:r0 + a.chunk]).sum()
        return hits.double() / z.shape[0]

    out, L = {}, _lib.load()
    for d in a.dims:
        g = torch.Generator(device=dev)
        g.manual_seed(d)
        y = torch.randint(0, a.classes, (a.n,), device=dev, generator=g)
        cen = torch.randn(a.classes, d, device=dev, generator=g)
        if d <= 256:          # codes: one Gaussian per class
            z = cen[y] + 1.5 * torch.randn(a.n, d, device=dev, generator=g)
        else:                 # pixels in [-1, 1]
            z = torch.tanh(0.05 * cen[y] + 0.5 * torch.randn(a.n, d, device=dev, generator=g))
        y32 = y.int()
        ways = dict(knn_accuracy=lambda: F.knn_accuracy(z, y32, k, a.classes), torch=lambda: torch_accuracy(z, y),
                    knn_radii=lambda: F.knn_radii(z, k))
        ours, ref = float(ways['knn_accuracy']().item()), float(ways['torch']().item())
        rec = dict(accuracy=ours, torch_accuracy=ref, abs_diff_to_torch=abs(ours - ref))
        for fn in ways.values():
            fn(); fn()
        torch.cuda.synchronize()
        times = {name: [] for name in ways}
        for _ in range(a.repeat):
            for name, fn in ways.items():
                times[name].append(window(fn))
        for name, ts in times.items():
            rec[('op_' if name != 'torch' else '') + name + ('_chunk%d' % a.chunk if name == 'torch' else '')] = dict(
                median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))
        med = {name: float(np.median(ts)) for name, ts in times.items()}
        rec['torch_over_knn_accuracy'] = med['torch'] / med['knn_accuracy']
        rec['knn_accuracy_over_knn_radii'] = med['knn_accuracy'] / med['knn_radii']
        L.ggan_prof_reset(); L.ggan_prof_enable(1)
        for _ in range(3):
            ways['knn_accuracy'](); ways['knn_radii']()
        torch.cuda.synchronize()
        rep = {r['name']: r for r in _lib.prof_report() if r['name'] in KERNELS}
        L.ggan_prof_enable(0)
        rec['kernels_ms'] = {name: r['total_ms'] / r['launches'] for name, r in rep.items()}
        for name in ('knn_lists', 'knn_radii'):
            rec['tflops_' + name] = rep[name]['flops'] / rep[name]['launches'] / (rec['kernels_ms'][name] * 1e-3) / 1e12
            rec['of_fp32_mfma_peak_' + name] = rec['tflops_' + name] / PEAK_TFLOPS
        rec['launch_flop'] = rep['knn_lists']['flops'] / rep['knn_lists']['launches']
        out['d%d' % d] = rec
        print('d = %d: %s' % (d, json.dumps(rec)))
        del z, y
    print(json.dumps(out))


if __name__ == '__main__':
    main()
