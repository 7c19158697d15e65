"""Time of the k-NN-ball ops (functional.knn_radii / ball_counts / prdc, csrc/knn_sets.hip) on an MI355X, for docs/KERNELS.md.

  python tools/prdc_time.py [--n 10000] [--k 5] [--dims 128 3072] [--repeat 7] [--chunk 2048]

Per width d: a real and a generated set of n rows each, every call warmed twice, then `prdc` (two radii sweeps, two count sweeps and the
four scores) timed `--repeat` times between HIP events (median, min, max printed), and `knn_radii` / `ball_counts` alone the same way.
Beside it what a user of torch would write: the same distances from `x @ y.T` and the row norms in row chunks of `--chunk`, so that no
n x n matrix is held, `kthvalue` per chunk for the radii (own index set to +inf first), a comparison and a row sum / row minimum per chunk
for the counts; the four scores of both paths are compared.  FLOP: the launches' own counts (tiles computed x 2 x 128 x 128 x d, the
figures they hand to the profiler) over the time, against the fp32-MFMA peak of 157.3 TFLOP/s; libggan's per-kernel timers give every
kernel's time alone.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3
KERNELS = ('knn_norms', 'knn_radii', 'knn_final', 'ball_norms', 'ball_counts', 'ball_final')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--dims', type=int, nargs='+', default=[128, 3072])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=2048)
    a = ap.parse_args()
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    k = a.k

    def timed(fn, reps):
        fn(); fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))

    def chunks(p, q):
        nq = (q * q).sum(1)
        for r0 in range(0, p.shape[0], a.chunk):
            pc = p[r0:r0 + a.chunk]
            yield r0, ((pc * pc).sum(1)[:, None] + nq[None, :] - 2.0 * (pc @ q.t())).clamp_(min=0)

    def torch_radii(z):
        out = []
        for r0, D in chunks(z, z):
            i = torch.arange(D.shape[0], device=dev)
            D[i, i + r0] = float('inf')
            out.append(D.kthvalue(k, dim=1).values)
        return torch.cat(out)

    def torch_counts(p, q, rq):
        cnt, mn = [], []
        for _, D in chunks(p, q):
            cnt.append((D <= rq[None, :]).sum(1))
            mn.append(D.min(1).values)
        return torch.cat(cnt), torch.cat(mn)

    def torch_prdc(x, y):
        r_x, r_y = torch_radii(x), torch_radii(y)
        cy, _ = torch_counts(y, x, r_x)
        cx, mx = torch_counts(x, y, r_y)
        f8 = torch.float64
        return torch.stack([(cy > 0).sum(dtype=f8), (cx > 0).sum(dtype=f8), cy.sum(dtype=f8) / k, (mx <= r_x).sum(dtype=f8)]) / x.shape[0]

    out, L = {}, _lib.load()
    for d in a.dims:
        g = torch.Generator(device=dev)
        g.manual_seed(d)
        if d <= 256:          # codes
            x, y = torch.randn(a.n, d, device=dev, generator=g), torch.randn(a.n, d, device=dev, generator=g) * 1.1 + 0.1
        else:                 # pixels in [-1, 1]
            x, y = torch.rand(a.n, d, device=dev, generator=g) * 2 - 1, torch.tanh(torch.randn(a.n, d, device=dev, generator=g))
        ours, ref = F.prdc(x, y, k).cpu().tolist(), torch_prdc(x, y).cpu().tolist()
        rec = dict(prdc=ours, abs_diff_to_torch=[abs(p - q) for p, q in zip(ours, ref)])
        r_x = F.knn_radii(x, k)
        rec['op_prdc'] = timed(lambda: F.prdc(x, y, k), a.repeat)
        rec['op_knn_radii'] = timed(lambda: F.knn_radii(x, k), a.repeat)
        rec['op_ball_counts'] = timed(lambda: F.ball_counts(y, x, r_x), a.repeat)
        rec['torch_chunk%d' % a.chunk] = timed(lambda: torch_prdc(x, y), max(3, a.repeat // 2))
        L.ggan_prof_reset(); L.ggan_prof_enable(1)
        for _ in range(3):
            F.prdc(x, y, k)
        torch.cuda.synchronize()
        rep = {r['name']: r for r in _lib.prof_report() if r['name'] in KERNELS}
        L.ggan_prof_enable(0)
        rec['kernels_ms'] = {name: r['total_ms'] / r['launches'] for name, r in rep.items()}
        flop = sum(r['flops'] / 3.0 for r in rep.values() if r['name'] in ('knn_radii', 'ball_counts'))      # per prdc call: 2 + 2 sweeps
        rec['launch_flop'] = flop
        rec['tflops'] = flop / (rec['op_prdc']['median_ms'] * 1e-3) / 1e12
        rec['of_fp32_mfma_peak'] = rec['tflops'] / PEAK_TFLOPS
        for name in ('knn_radii', 'ball_counts'):
            rec['tflops_' + name] = rep[name]['flops'] / rep[name]['launches'] / (rec['kernels_ms'][name] * 1e-3) / 1e12
        out['d%d' % d] = rec
        print('d = %d: %s' % (d, json.dumps(rec)))
        del x, y
    print(json.dumps(out))


if __name__ == '__main__':
    main()
